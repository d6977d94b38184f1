"""The ground plan view (include/svo.h, "Ground plan view") against its restatement tests/grid_view_ref.py, with == on all
n_views records, order, best, seen and all eight counts.

CPU: the restatement's two routes (cell by cell in Python integers, whole arrays in numpy) agree on every case used below but those
with max_range >= 63, which only the numpy route covers; the random cases between them have one with less than half of the targets in
range visible and one with more than 90 %, a cell that the corner rule decides, a cell that a tie of rule 3 decides and a list with
ignored views of all three kinds; the constructed grids are what they were built to be; each deliberate misreading of the contract
changes a stated case by a stated count; the pure entries and the refusals that need no context; stereo_vo_amd/host/view_args.h walked
by tests/sanitize/grid_view_args_test.cpp under ASan + UBSan.
GPU: seeded grids of 1 x 1, 1 x 70, 70 x 1, 17 x 17 (smaller than the window: all four edges clip), 63 x 65 and 130 x 300 at max_range
1, 2, 15, 16, 31, 32 (window rows of 31, 33, 63 and 65 bits), 64 and, with eight views on 130 x 300, 255; views in the four corners;
n_views 1, 64 with duplicates and padding, 4096 at max_range 3; a list that is all ignored; with and without cost, masks that share the
UNKNOWN bit and masks that do not; each output left out alone, no counts, a repeated call and the unstaged mode byte for byte; the
score's two ends; every refusal with zero brackets; the constructed grids through both entries.  Every device call runs into a dirty
workspace and sentinel-filled outputs whose guard elements stay, with cls, views and cost between guard elements.

Misreadings, what changes on the restatement (grid "misreading": 63 x 65, obstacle density 0.15, seed 7, 12 views at max_range 12 with
cost; 9 used, 3,126 targets in range, 1,252 visible, 854 cells covered):
  a tie rounded towards V 79 cells of seen; range < 4 seen; an OPAQUE target not visible 124 seen; sight through closed corners 48 seen; a
  diagonal step blocked by either side cell 314 seen; no occlusion 976 seen; V not counted 9 n_visible; an ignored view left out of order
  3 order; order ties to the largest index 6 order; a NONE cost taken as 0 1 score; a score that wraps 1 score.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import grid_view_ref as G
from test_host_sanitizers import _run_sanitized

MISREADINGS = {"tie_towards": ("seen", 79), "range_lt": ("seen", 4), "opaque_target_hidden": ("seen", 124), "open_corners": ("seen", 48),
               "either_corner": ("seen", 314), "no_occlusion": ("seen", 976), "no_self": ("n_visible", 9), "order_drop_ignored": ("order", 3),
               "order_largest": ("order", 6), "none_zero": ("score", 1), "score_wraps": ("score", 1)}
OUTPUTS = ("records", "order", "best", "seen")
DENSITIES = ((0.3, 0.02), (0.3, 0.05), (0.3, 0.15))  # (p_unknown, p_obstacle)
BIG = (130, 300)
# (na, nb, max_range, n_views, density, with_cost, shared masks): the smallest shapes at which the kernel can go wrong
RANDOM = [(1, 1, 1, 1, 0, True, False), (1, 1, 2, 8, 1, False, False),
          (1, 70, 1, 8, 0, True, False), (1, 70, 16, 8, 1, False, True), (1, 70, 64, 8, 2, True, False),
          (70, 1, 2, 8, 2, True, True), (70, 1, 15, 8, 0, False, False), (70, 1, 32, 8, 1, True, False)] + \
         [(17, 17, r, 8, k % 3, k % 2 == 0, k % 4 == 1) for k, r in enumerate((1, 2, 15, 16, 31, 32, 64))] + \
         [(63, 65, 15, 64, 0, True, False), (63, 65, 16, 64, 2, True, True), (63, 65, 31, 16, 1, False, False), (63, 65, 32, 16, 2, True, False),
          (63, 65, 64, 16, 0, True, True), (63, 65, 5, 1, 1, True, False)] + \
         [(*BIG, 2, 64, 2, True, False), (*BIG, 31, 16, 0, True, False), (*BIG, 32, 16, 1, False, True), (*BIG, 64, 16, 2, True, False),
          (*BIG, 255, 8, 1, True, False), (63, 65, 3, 4096, 1, True, False)]
CORNERS = [(17, 17, 2), (17, 17, 32), (63, 65, 16), (*BIG, 64)]
MODES = [(c, s) for c in (False, True) for s in (False, True)]


def _freeze(r):
    for a in (r.records, r.order, r.best, r.seen):
        a.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def random_want(na, nb, max_range, n_views, density, with_cost, shared, seed=None):
    case = G.random_case(na, nb, *DENSITIES[density], n_views, max_range, seed=seed, with_cost=with_cost, **(G.SHARED if shared else {}))
    stats = {}
    return case, _freeze(G.views_np(*case, stats=stats)), stats


@functools.lru_cache(maxsize=None)
def corner_want(na, nb, max_range):
    case = G.corner_case(na, nb, max_range)
    return case, _freeze(G.views_np(*case))


@functools.lru_cache(maxsize=None)
def constructed_want():
    return {name: (case, _freeze(G.views_np(*case)), facts) for name, (case, facts) in G.constructed().items()}


@functools.lru_cache(maxsize=None)
def ignored_want():
    """a list that is all ignored: padding, outside the grid, in a wall"""
    case = random_want(63, 65, 16, 64, 2, True, False)[0]
    wall = int(np.flatnonzero(case.cls.ravel() == G.OBSTACLE)[0])
    case = case._replace(views=np.array([G.NONE, 63 * 65, wall, 1 << 31, wall, G.NONE], np.uint32))
    return case, _freeze(G.views_np(*case))


@functools.lru_cache(maxsize=None)
def score_want():
    """300 x 300 of UNKNOWN ground that is looked through, but for four LEVEL cells, one of them boxed in; max_range 255, gain_weight
    65536, cost_div 1: the middle view gains more than 65,536 cells (the clamp at 0xFFFFFFFE, a cost beneath it), the boxed view gains 0
    against a cost of 5 and the corner view tens of thousands of cells against a cost of 0xFFFFFFF0 (0 both, not wrapped), the last
    has no way there (0)."""
    n = 300
    cls = np.full((n, n), G.UNKNOWN, np.uint8)
    mid, boxed, corner, lost = 150 * n + 150, 5 * n + 5, n * n - 1, 290 * n + 290
    cls[4:7, 4:7] = G.OBSTACLE
    for v in (mid, boxed, corner, lost):
        cls.ravel()[v] = G.LEVEL
    cost = np.zeros((n, n), np.uint32)
    cost.ravel()[[mid, boxed, corner, lost]] = [12345, 5, 0xFFFFFFF0, G.NONE]
    case = G.Case(cls, np.array([mid, boxed, corner, lost], np.uint32), cost, G.params(cls, max_range=255, gain_weight=65536, cost_div=1))
    return case, _freeze(G.views_np(*case))


# ===================================================================================================== CPU
def test_the_two_routes_of_the_restatement_agree_on_every_case_both_cover():
    covered = 0
    for key in RANDOM:
        case, a, _ = random_want(*key)
        if case.prm.max_range <= G.PY_MAX_RANGE:
            covered += 1
            assert G.same(a, G.views_py(*case)), key
    assert covered == len(RANDOM) - 5  # max_range 64 four times and 255 once
    for key in CORNERS:
        case, a = corner_want(*key)
        if case.prm.max_range <= G.PY_MAX_RANGE:
            assert G.same(a, G.views_py(*case)), key
    for cost, shared in MODES:
        case, a, _ = random_want(63, 65, 16, 64, 1, cost, shared, 11)
        assert G.same(a, G.views_py(*case)), (cost, shared)
    for name, (case, a, _) in constructed_want().items():
        assert G.same(a, G.views_py(*case)), name
    case, a = ignored_want()
    assert G.same(a, G.views_py(*case))
    case = G.misreading_case()
    assert G.same(G.views_np(*case), G.views_py(*case))


def test_the_random_cases_are_what_the_kernels_paths_need():
    """Conditions on the inputs, asserted on the restatement alone."""
    shares = {}
    for key in RANDOM:
        case, a, stats = random_want(*key)
        if a.counts[2]:
            shares[key] = a.counts[3] / a.counts[2]
        assert stats["targets"] == a.counts[2] and a.counts[3] == int(a.records["n_visible"].sum()) and a.counts[4] == int(a.records["n_gain"].sum())
        assert a.counts[0] + a.counts[1] == len(case.views) and a.counts[6] <= a.counts[5] <= min(a.counts[3], case.prm.na * case.prm.nb)
        assert sorted(a.order.tolist()) == list(range(len(case.views)))
    print("visible shares", sorted(round(s, 3) for s in shares.values()))
    assert min(shares.values()) < 0.5 and max(shares.values()) > 0.9
    # the corner rule and a tie of rule 3 each decide a cell of a random case
    case, a, _ = random_want(63, 65, 16, 64, 2, True, True)
    assert int((G.views_np(*case, variant="open_corners").seen != a.seen).sum()) > 0
    assert int((G.views_np(*case, variant="tie_towards").seen != a.seen).sum()) > 0
    # ignored views of all three kinds in one list, beside duplicates
    n = case.prm.na * case.prm.nb
    v = case.views
    walls = {int(x) for x in v if x < n and case.cls.ravel()[x] == G.OBSTACLE}
    assert (v == G.NONE).any() and ((v >= n) & (v != G.NONE)).any() and walls
    used = v[a.records["cell"] != G.NONE]
    assert len(set(used.tolist())) < len(used) and a.counts[1] >= 3 and a.counts[0] > 32
    # scores on both sides of the cost, an unreachable view, and a tie that the index breaks
    s = a.records["score"][a.records["cell"] != G.NONE]
    assert (s == 0).any() and (s > 0).any() and (a.records["cost"][a.records["cell"] != G.NONE] == G.NONE).any()
    assert len(set(s[s > 0].tolist())) < int((s > 0).sum())


def test_the_constructed_grids_are_what_they_were_built_to_be():
    for name, (case, a, facts) in constructed_want().items():
        if "counts" in facts:
            assert tuple(a.counts) == facts["counts"], (name, a.counts)
        for i, fields in facts.get("records", {}).items():
            for f, v in fields.items():
                assert int(a.records[i][f]) == v, (name, i, f, int(a.records[i][f]))
        for at in facts.get("visible", []):
            assert int(a.seen[at]) == 0, (name, at)
        for at in facts.get("hidden", []):
            assert int(a.seen[at]) == G.NONE, (name, at)
        if "order" in facts:
            assert a.order.tolist() == facts["order"], name
        if "best" in facts:
            assert tuple(a.best.tolist()) == facts["best"], name
    cw = constructed_want()
    for name in ("closed_room", "diamond_room"):  # nothing outside the wall is visible
        case, a, _ = cw[name]
        wall = case.cls == G.OBSTACLE
        assert not (a.seen[case.cls == G.UNKNOWN] != G.NONE).any() and int((a.seen[wall] == 0).sum()) == int(a.records[0]["n_opaque"]), name
    case, a, _ = cw["diamond_room"]
    leak = G.views_np(*case, variant="open_corners")
    assert int(leak.records[0]["n_gain"]) > 0 and int(a.records[0]["n_gain"]) == 0  # only the corner rule closes it
    case, a, _ = cw["door"]
    beyond = a.seen[:, 7:] == 0
    assert beyond[5].all() and beyond.sum() == int(a.records[0]["n_gain"]) == int(a.counts[6])
    case, a, _ = cw["tie_blocked"]
    assert int(G.views_np(*case, variant="tie_towards").seen[2, 1]) == 0  # a line drawn from T sees it
    case, a = score_want()
    ng = a.records["n_gain"].tolist()
    assert a.records["score"].tolist() == [G.MAX_SCORE, 0, 0, 0] and ng[0] > 65536 and ng[1] == 0 and 0 < 65536 * ng[2] < 0xFFFFFFF0 and ng[3] > 0
    assert a.order.tolist() == [0, 1, 2, 3] and a.best.tolist() == [150 * 300 + 150, 0, G.MAX_SCORE, ng[0]]


def test_every_misreading_of_the_contract_changes_a_stated_case():
    case = G.misreading_case()
    right = G.views_np(*case)
    assert right.counts[:4] == (9, 3, 3126, 1252) and right.counts[5] == 854
    got = {}
    for variant, (field, _) in MISREADINGS.items():
        wrong = G.views_np(*case, variant=variant)
        if field in ("seen", "order"):
            got[variant] = (field, int((getattr(wrong, field) != getattr(right, field)).sum()))
        else:
            got[variant] = (field, int((wrong.records[field] != right.records[field]).sum()))
        assert got[variant][1] > 0, variant
    assert got == MISREADINGS, got
    assert set(MISREADINGS) == set(G.VARIANTS)


def _api_params(prm):
    from stereo_vo_amd import api
    return api.GridViewParams(*prm)


def test_pure_entries_and_refusals_without_a_context():
    from stereo_vo_amd import api
    L = api.lib()
    g = api.voxel_grid_default_params(0.1)
    cp = api.grid_clearance_default_params(g, 0.1)
    d = api.grid_view_default_params(cp)
    assert (d.na, d.nb, d.opaque_mask, d.gain_mask, d.max_range, d.gain_weight, d.cost_div) == \
        (256, 256, 1 << api.VOXEL_GRID_OBSTACLE, 1 << api.VOXEL_GRID_UNKNOWN, 64, 16, 1)
    cp.na, cp.nb, cp.max_dist = 17, 300, 8191
    d = api.grid_view_default_params(cp)
    assert (d.na, d.nb, d.max_range) == (17, 300, 255)
    cp.max_dist = 255
    assert api.grid_view_default_params(cp).max_range == 255
    cp.max_dist = 7
    assert api.grid_view_default_params(cp).max_range == 7
    for field, value in (("na", 0), ("nb", 8193), ("na", 8192)):  # 8192 x 2049 is beyond 2^24
        bad = api.GridClearanceParams(17, 2049, 4, 64, 0.5, 0.0)
        setattr(bad, field, value)
        with pytest.raises(api.SvoError):
            api.grid_view_default_params(bad)
    assert L.svo_grid_view_default_params(None, C.byref(d)) == -1 and L.svo_grid_view_default_params(C.byref(cp), None) == -1
    ws = api.grid_view_workspace_bytes
    assert ws(0, 5, 1) == 0 and ws(5, -1, 1) == 0 and ws(5, 5, 0) == 0 and ws(5, 5, 4097) == 0 and ws(8192, 2049, 1) == 0 and ws(40000, 40000, 1) == 0
    r8 = lambda b: (b + 7) // 8 * 8
    for na, nb, nv in ((1, 1, 1), (15, 17, 64), (256, 256, 1024), (130, 300, 4096), (8192, 2048, 4096)):
        assert ws(na, nb, nv) == 256 + 16 * nv + r8(4 * na * nb) and ws(na, nb, nv) % 8 == 0
    assert api.GRID_VIEW_NONE == 0xFFFFFFFF and api.GRID_VIEW_DTYPE == G.RECORD and C.sizeof(api.GridViewParams) == 28
    assert len(api.GRID_VIEW_COUNTS) == 7 and api.GRID_VIEW_MAX_VIEWS == 4096
    # a null context is refused by every entry before anything else is looked at
    buf = (C.c_double * 12)()
    out = api.GridViewOut(C.addressof(buf))
    assert L.svo_grid_view_dev(None, buf, buf, 1, None, C.byref(d), buf, C.byref(out), None) == -1
    assert L.svo_grid_view(None, buf, buf, 1, None, C.byref(d), C.byref(out), None) == -1
    assert L.svo_grid_view_dev(None, None, None, 0, None, None, None, None, None) == -1
    assert L.svo_grid_view_set_mode(None, 1) == -1


def test_grid_view_args_every_refusal_the_sizes_the_rings_and_the_defaults(tmp_path):
    """host/view_args.h on the CPU under ASan + UBSan: every refusal at its boundary with code and exact message, the order of the
    refusals, the workspace's size and layout, the window's words, the ring enumeration (every offset of the square visited exactly
    once for max_range 1, 2, 31, 32 and 255, ring by ring), the score at its edges, the defaults."""
    _run_sanitized(tmp_path, "grid_view_args_test", "grid view args ok")


# ===================================================================================================== GPU
_SENT = {"records": (np.int64, 0x5A5A5A5A5A5A5A5A), "order": (np.int32, 0x3333CCCC), "best": (np.int32, 0x77771111), "seen": (np.int32, 0x5555AAAA)}


class _Dev:
    """A case's device buffers: cls, views and cost between guard elements, a dirty workspace and sentinel-filled outputs with a guard
    element before and behind each.  skip: of OUTPUTS, the outputs passed as NULL."""

    def __init__(self, case, skip=(), counts=True):
        import torch
        from stereo_vo_amd import api
        self.case, self.prm, self.skip, self.counts = case, case.prm, tuple(skip), counts
        n, nv = self.prm.na * self.prm.nb, len(case.views)
        self.n, self.nv = n, nv

        def guarded(a, t, guard):
            d = torch.full((len(a) + 2,), guard, dtype=t, device="cuda")
            d[1:-1] = torch.from_numpy(np.ascontiguousarray(a)).cuda()
            return d

        # a guard read as a cell would be UNKNOWN and cheap, a guard read as a view would be cell 0
        self.cls = guarded(case.cls.ravel(), torch.uint8, G.UNKNOWN)
        self.views = guarded(case.views.view(np.int32), torch.int32, 0)
        self.cost = None if case.cost is None else guarded(case.cost.ravel().view(np.int32), torch.int32, 0)
        words = api.grid_view_workspace_bytes(self.prm.na, self.prm.nb, nv) // 8
        assert words > 0
        self.ws = torch.full((words + 2,), 0x7F7F7F7F7F7F7F7F, dtype=torch.int64, device="cuda")
        sizes = {"records": 4 * nv, "order": nv, "best": 4, "seen": n}
        self.bufs = {k: torch.full((sizes[k] + 2,), v, dtype=getattr(torch, np.dtype(t).name), device="cuda") for k, (t, v) in _SENT.items()}
        self.cnt = torch.full((10,), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()

    def call(self, ctx, **over):
        p = _api_params(self.prm._replace(**over))
        ptr = {k: None if k in self.skip else b.data_ptr() + b.element_size() for k, b in self.bufs.items()}
        out = ctx.grid_view(self.cls.data_ptr() + 1, self.views.data_ptr() + 4, self.nv, p, cost_ptr=None if self.cost is None else self.cost.data_ptr() + 4,
                            workspace_ptr=self.ws.data_ptr() + 8, counts_ptr=self.cnt.data_ptr() + 8 if self.counts else None,
                            **{k + "_ptr": v for k, v in ptr.items()})
        assert out["seen"] == ptr["seen"] and (out["na"], out["nb"], out["n_views"]) == (self.prm.na, self.prm.nb, self.nv)
        ctx.sync()

    def read(self, keep=None):
        """{"records", "order", "best", "seen", "counts": the eight}, None for what was skipped"""
        case, prm = self.case, self.prm
        w = self.ws.cpu().numpy()
        assert w[0] == w[-1] == 0x7F7F7F7F7F7F7F7F
        assert np.array_equal(self.cls.cpu().numpy()[1:-1].reshape(case.cls.shape), case.cls)  # only read
        assert np.array_equal(self.views.cpu().numpy()[1:-1].view(np.uint32), case.views)
        if self.cost is not None:
            assert np.array_equal(self.cost.cpu().numpy()[1:-1].view(np.uint32).reshape(case.cls.shape), case.cost)
        got = {}
        for k, (t, v) in _SENT.items():
            a = self.bufs[k].cpu().numpy()
            assert a[0] == v and a[-1] == v, k  # nothing beside the outputs is written
            if k in self.skip:
                assert (a == v).all(), k
                got[k] = None
            else:
                got[k] = a[1:-1]
            if keep is not None:
                keep[k] = a.tobytes()
        c = self.cnt.cpu().numpy()
        assert c[0] == c[-1] == -1 and (self.counts or (c == -1).all())
        got["counts"] = tuple(int(v) for v in c[1:9]) if self.counts else None
        if keep is not None:
            keep["counts"] = c.tobytes()
        if got["records"] is not None:
            got["records"] = got["records"].view(G.RECORD)
        for k in ("order", "best"):
            if got[k] is not None:
                got[k] = got[k].view(np.uint32)
        if got["seen"] is not None:
            got["seen"] = got["seen"].view(np.uint32).reshape(prm.na, prm.nb)
        return got


def _eq(got, w, what=""):
    if got["counts"] is not None:
        assert got["counts"] == tuple(w.counts) + (0,), (what, got["counts"], w.counts)
    if got["records"] is not None:
        rec = got["records"]
        bad = [i for i in range(len(w.records)) if rec[i] != w.records[i]]
        assert not bad, (what, "records", bad[:4], rec[bad[0]], w.records[bad[0]])
    for k in ("order", "best", "seen"):
        if got[k] is not None:
            assert np.array_equal(got[k], getattr(w, k)), (what, k, int((got[k] != getattr(w, k)).sum()), got[k].ravel()[:8], getattr(w, k).ravel()[:8])


def _run(ctx, case, how="dev", skip=(), counts=True, keep=None):
    if how == "host":
        from stereo_vo_amd import api
        r = ctx.grid_view_host(case.cls, case.views, case.cost, _api_params(case.prm))
        assert tuple(r["counts"]) == api.GRID_VIEW_COUNTS and tuple(r["best"]) == api.GRID_VIEW_BEST
        return {"records": r["records"], "order": r["order"], "best": np.array(list(r["best"].values()), np.uint32), "seen": r["seen"],
                "counts": tuple(r["counts"].values()) + (0,)}
    d = _Dev(case, skip, counts)
    d.call(ctx)
    return d.read(keep)


@pytest.mark.gpu
@pytest.mark.parametrize("key", RANDOM, ids=lambda k: "-".join(str(int(x)) for x in k))
def test_random_grids(ctx, key):
    case, w, stats = random_want(*key)
    got = _run(ctx, case)
    print(key, "counts", got["counts"], "steps per target", stats["steps"] / max(stats["targets"], 1))
    _eq(got, w, key)


@pytest.mark.gpu
def test_views_in_the_four_corners(ctx):
    for key in CORNERS:
        case, w = corner_want(*key)
        assert w.counts[0] == 5
        got = _run(ctx, case)
        print(key, got["counts"])
        _eq(got, w, key)


@pytest.mark.gpu
def test_constructed_grids_through_both_entries(ctx):
    for name, (case, w, facts) in constructed_want().items():
        for how in ("dev", "host"):
            got = _run(ctx, case, how)
            print(name, how, got["counts"])
            _eq(got, w, (name, how))


@pytest.mark.gpu
def test_with_and_without_cost_shared_and_separate_masks(ctx):
    seen = set()
    for cost, shared in MODES:
        case, w, _ = random_want(63, 65, 16, 64, 1, cost, shared, 11)
        _eq(_run(ctx, case), w, (cost, shared))
        _eq(_run(ctx, case, "host"), w, (cost, shared, "host"))
        seen.add(w.records.tobytes())
    assert len(seen) == 4


@pytest.mark.gpu
def test_a_list_that_is_all_ignored(ctx):
    case, w = ignored_want()
    assert w.counts == (0, 6, 0, 0, 0, 0, 0) and w.best.tolist() == [G.NONE, G.NONE, 0, 0] and w.order.tolist() == list(range(6)) and (w.seen == G.NONE).all()
    _eq(_run(ctx, case), w)
    _eq(_run(ctx, case, "host"), w, "host")


@pytest.mark.gpu
def test_the_scores_two_ends(ctx):
    case, w = score_want()
    got = _run(ctx, case)
    print(got["records"], got["counts"])
    _eq(got, w)
    case2 = case._replace(cost=None)
    _eq(_run(ctx, case2), G.views_np(*case2), "no cost")


@pytest.mark.gpu
def test_optional_outputs_no_counts_a_repeated_call_and_the_unstaged_mode(ctx):
    case, w, _ = random_want(63, 65, 16, 64, 2, True, True)
    for skip in [(k,) for k in OUTPUTS] + [("records", "order", "best"), ("order", "best", "seen"), ("records", "order", "seen")]:
        got = _run(ctx, case, skip=skip)
        assert all((got[k] is None) == (k in skip) for k in OUTPUTS)
        _eq(got, w, skip)
    _eq(_run(ctx, case, counts=False), w, "no counts")
    _eq(_run(ctx, case, skip=("records", "order", "seen"), counts=False), w, "best alone")
    _eq(_run(ctx, case, skip=("seen",), counts=False), w, "neither seen nor counts")
    # the host entry: keywords instead of a parameter set, and single outputs
    r = ctx.grid_view_host(case.cls, case.views, cost=case.cost, max_range=16, **G.SHARED)
    assert r["records"].tobytes() == w.records.tobytes() and np.array_equal(r["seen"], w.seen) and tuple(r["counts"].values()) == tuple(w.counts)
    from stereo_vo_amd import api
    best = np.full(4, 0x77771111, np.uint32)
    p = _api_params(case.prm)
    assert ctx.L.svo_grid_view(ctx.h, case.cls.ctypes.data, case.views.ctypes.data, len(case.views), case.cost.ctypes.data, C.byref(p),
                               C.byref(api.GridViewOut(None, None, best.ctypes.data, None)), None) == 0
    assert np.array_equal(best, w.best)
    # twice: the same bytes in every output; once more with every step reading cls from global memory: the same bytes again
    for key in [(*BIG, 64, 16, 2, True, False), (*BIG, 255, 8, 1, True, False), (17, 17, 32, 8, 2, False, True), (63, 65, 3, 4096, 1, True, False)]:
        first, second, plain = {}, {}, {}
        big, wb, _ = random_want(*key)
        _eq(_run(ctx, big, keep=first), wb)
        _eq(_run(ctx, big, keep=second), wb)
        ctx.grid_view_set_mode(False)
        try:
            _eq(_run(ctx, big, keep=plain), wb, "unstaged")
        finally:
            ctx.grid_view_set_mode(None)
        assert first == second == plain and set(first) == set(_SENT) | {"counts"}


@pytest.mark.gpu
def test_the_unstaged_mode_on_every_small_shape(ctx):
    ctx.grid_view_set_mode(False)
    try:
        for key in RANDOM:
            if key[0] * key[1] <= 17 * 17:
                case, w, _ = random_want(*key)
                _eq(_run(ctx, case), w, key)
    finally:
        ctx.grid_view_set_mode(None)


@pytest.mark.gpu
def test_bad_calls_launch_nothing_and_leave_the_context_usable(ctx):
    from stereo_vo_amd import api
    L = ctx.L
    case, w, _ = random_want(63, 65, 16, 64, 2, True, True)
    good = case.prm
    d = _Dev(case)
    O = api.GridViewOut
    P = {k: b.data_ptr() + b.element_size() for k, b in d.bufs.items()}
    full = lambda **kw: O(**{**P, **kw})
    A = dict(cls=d.cls.data_ptr() + 1, views=d.views.data_ptr() + 4, nv=d.nv, cost=d.cost.data_ptr() + 4, ws=d.ws.data_ptr() + 8, counts=d.cnt.data_ptr() + 8)

    def dev(prm=good, out=None, null_prm=False, null_out=False, **kw):
        a = {**A, **kw}
        o = out if out is not None else full()
        p = _api_params(prm)
        return L.svo_grid_view_dev(ctx.h, a["cls"], a["views"], a["nv"], a["cost"], None if null_prm else C.byref(p), a["ws"],
                                   None if null_out else C.byref(o), a["counts"])

    r = good._replace
    hseen = np.full((good.na, good.nb), 0x5555AAAA, np.uint32)

    def host(prm=good, cls=case.cls.ctypes.data, views=case.views.ctypes.data, nv=len(case.views), out=None, null_out=False, null_prm=False):
        o = out if out is not None else O(None, None, None, hseen.ctypes.data)
        return L.svo_grid_view(ctx.h, cls, views, nv, None, None if null_prm else C.byref(_api_params(prm)), None if null_out else C.byref(o), None)

    none = O(None, None, None, None)
    calls = [(lambda: dev(cls=None), "null cls"), (lambda: dev(null_prm=True), "null params"), (lambda: dev(views=None), "null views"),
             (lambda: dev(ws=None), "null workspace"), (lambda: dev(null_out=True), "null out"),
             (lambda: dev(r(na=0), ws=None), "null workspace"),  # the nulls before the ranges
             (lambda: dev(r(na=0)), "na outside"), (lambda: dev(r(na=8193)), "na outside"), (lambda: dev(r(nb=0)), "nb outside"),
             (lambda: dev(r(nb=8193)), "nb outside"), (lambda: dev(r(na=8192, nb=2049)), "na * nb"),
             (lambda: dev(r(opaque_mask=0)), "opaque_mask is 0"), (lambda: dev(r(gain_mask=0)), "gain_mask is 0"),
             (lambda: dev(r(max_range=0)), "max_range"), (lambda: dev(r(max_range=256)), "max_range"),
             (lambda: dev(r(gain_weight=0)), "gain_weight"), (lambda: dev(r(gain_weight=65537)), "gain_weight"),
             (lambda: dev(r(cost_div=0)), "cost_div"), (lambda: dev(r(cost_div=(1 << 31) + 1)), "cost_div"),
             (lambda: dev(nv=0), "n_views"), (lambda: dev(nv=4097), "n_views"), (lambda: dev(nv=-1), "n_views"),
             (lambda: dev(r(cost_div=0), nv=0), "cost_div"),  # the fields before n_views
             (lambda: dev(out=none), "all null"), (lambda: dev(out=none, nv=0), "n_views"),
             (lambda: dev(views=A["views"] + 2), "views must be 4-byte"), (lambda: dev(cost=A["cost"] + 2), "cost must be 4-byte"),
             (lambda: dev(out=full(order=P["order"] + 1)), "order must be 4-byte"), (lambda: dev(out=full(best=P["best"] + 2)), "best must be 4-byte"),
             (lambda: dev(out=full(seen=P["seen"] + 3)), "seen must be 4-byte"),
             (lambda: dev(out=full(records=P["records"] + 4)), "records must be 8-byte"),
             (lambda: dev(ws=A["ws"] + 4), "workspace must be 8-byte"), (lambda: dev(counts=A["counts"] + 4), "counts must be 8-byte"),
             (lambda: dev(cost=A["cost"] + 2, counts=A["counts"] + 4), "cost must be 4-byte"),  # the 4-byte ones first
             (lambda: host(cls=None), "null cls"), (lambda: host(null_prm=True), "null params"), (lambda: host(views=None), "null views"),
             (lambda: host(null_out=True), "null out"), (lambda: host(r(max_range=0)), "max_range"), (lambda: host(nv=4097), "n_views"),
             (lambda: host(out=none), "all null")]
    ctx.profile_select("grid_view")
    for call, word in calls:
        assert call() == -1 and word in L.svo_last_error(ctx.h).decode(), (word, L.svo_last_error(ctx.h).decode())
    assert ctx.profile_read()[1] == 0
    ctx.sync()
    for k, (t, v) in _SENT.items():
        assert (d.bufs[k].cpu().numpy() == v).all(), k
    assert (d.ws.cpu().numpy() == 0x7F7F7F7F7F7F7F7F).all() and (d.cnt.cpu().numpy() == -1).all() and (hseen == 0x5555AAAA).all()
    # the boundaries' accepted sides in one call: one bracket
    assert dev(r(max_range=255, gain_weight=65536, cost_div=1 << 31, opaque_mask=0x80000004, gain_mask=0x80000001), cost=None, counts=None,
               out=full(records=None, seen=None)) == 0
    assert ctx.profile_read()[1] == 1
    ctx.profile_select(None)
    with pytest.raises(api.SvoError):
        ctx.grid_view(A["cls"], A["views"], d.nv, _api_params(good), seen_ptr=P["seen"])  # no workspace
    with pytest.raises(api.SvoError):
        ctx.grid_view_host(case.cls, case.views, max_range=0)
    with pytest.raises(api.SvoError):
        ctx.grid_view_host(case.cls, np.zeros(0, np.uint32))
    with pytest.raises(ValueError):
        ctx.grid_view_host(case.cls, case.views, params=_api_params(good._replace(na=5)))
    with pytest.raises(ValueError):
        ctx.grid_view_host(case.cls, case.views, cost=case.cost[:5])
    # the context is what it was, and gives the view
    _eq(_run(ctx, case), w)
    _eq(_run(ctx, case, "host"), w)
