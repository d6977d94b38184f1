"""The ground plan frontiers (include/svo.h, "Ground plan frontiers") against their restatement tests/grid_frontier_ref.py,
with == on the records up to n_written, goal_cells over all max_frontiers entries, label and all eight counts.

CPU: the restatement's two routes (flood fill in Python integers, whole arrays in numpy) agree on every case used below; the random
cases between them give many small frontiers, one that spans every tile and more kept frontiers than a small max_frontiers; the
constructed grids are what they were built to be; each deliberate misreading of the contract changes a stated case by a stated count;
the pure entries and the refusals that need no context; stereo_vo_amd/host/frontier_args.h walked by
tests/sanitize/grid_frontier_args_test.cpp under ASan + UBSan.
GPU: seeded grids of seventeen shapes at three densities, each with and without blocked and with and without cost; the constructed
grids through both entries; max_frontiers 1, 64 and 4096; min_size 1 and 2^24; each output left out alone, no counts; a repeated call;
the combining of runs turned off; bad calls.  Every device call runs into a dirty workspace and sentinel-filled outputs whose guard
elements stay, with cls, blocked and cost between guard elements; records past n_written still hold the sentinel.

Misreadings, what changes on the restatement (grid "misreading": 63 x 65, densities (0.3, 0.1), seed 7, blocked and cost, min_size 3;
1,752 frontier cells in 37 frontiers, 7 kept):
  four-connected components 1,707 labels; the eight-neighbour UNKNOWN test 2,124 labels; blocked ignored 1,813 labels; the outside read as
  unknown 1,741 labels; size > min_size 15 labels; rank by size 1,711 labels; the centroid rounded 3 rep_cell; the rep_cell tie to the
  largest index 3 rep_cell; the best_cell tie to the largest index 1 best_cell; a NONE cost taken as the smallest 6 best_cell.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import grid_frontier_ref as G
from test_host_sanitizers import _run_sanitized

MISREADINGS = {"four": ("label", 1707), "eight_unknown": ("label", 2124), "no_blocked": ("label", 1813), "outside_unknown": ("label", 1741),
               "gt_min": ("label", 15), "rank_size": ("label", 1711), "round_centroid": ("rep_cell", 3), "rep_largest": ("rep_cell", 3),
               "best_largest": ("best_cell", 1), "none_smallest": ("best_cell", 6)}
OUTPUTS = ("frontiers", "goal_cells", "label")
BIG = (130, 300)


def _freeze(r):
    for a in r[:3]:
        a.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def random_want(na, nb, density, with_blocked, with_cost, min_size=3, max_frontiers=1024):
    case = G.random_case(na, nb, *density, with_blocked=with_blocked, with_cost=with_cost, min_size=min_size, max_frontiers=max_frontiers)
    return case, _freeze(G.frontiers_np(*case))


@functools.lru_cache(maxsize=None)
def constructed_want():
    return {name: (case, _freeze(G.frontiers_np(*case)), facts) for name, (case, facts) in G.constructed().items()}


RANDOM = [(na, nb, density, b, c) for na, nb in G.SIZES for density in G.DENSITIES for b in (False, True) for c in (False, True)]
TRUNCATED = [(density, mf) for density in G.DENSITIES for mf in (1, 64, 4096)]
MIN_SIZES = (1, 1 << 24)


# ===================================================================================================== CPU
def test_the_two_routes_of_the_restatement_agree_on_every_case():
    for na, nb, density, b, c in RANDOM:
        case, a = random_want(na, nb, density, b, c)
        assert G.same(a, G.frontiers_py(*case)), (na, nb, density, b, c)
    for density, mf in TRUNCATED:
        case, a = random_want(*BIG, density, True, True, 3, mf)
        assert G.same(a, G.frontiers_py(*case)), (density, mf)
    for ms in MIN_SIZES:
        case, a = random_want(63, 65, G.DENSITIES[1], True, True, ms)
        assert G.same(a, G.frontiers_py(*case)), ms
    for name, (case, a, _) in constructed_want().items():
        assert G.same(a, G.frontiers_py(*case)), name
    case = G.misreading_case()
    assert G.same(G.frontiers_np(*case), G.frontiers_py(*case))


def test_the_random_cases_are_what_the_kernels_paths_need():
    """Conditions on the inputs, asserted on the restatement alone: many small frontiers, one that spans every tile, more kept frontiers
    than a small max_frontiers and fewer."""
    cells = kept = largest = 0
    n_kept = []
    for na, nb, density, b, c in RANDOM:
        if not (b and c):
            continue
        case, a = random_want(na, nb, density, b, c, 3, 65536 if (na, nb) == BIG else 1024)
        assert a.counts[5] == a.counts[4]  # nothing truncated here
        assert sum(int(s) for s in a.frontiers["size"]) == a.counts[6] and a.counts[2] >= a.counts[6]
        cells += a.counts[2]
        kept += a.counts[4]
        n_kept.append(a.counts[4])
        largest = max(largest, int(a.frontiers["size"].max()) if len(a.frontiers) else 0)
    print("frontier cells", cells, "kept", kept, "largest", largest)
    assert cells > 20000 and kept > 1000 and largest > 10000
    assert any(k > 64 for k in n_kept) and any(0 < k <= 64 for k in n_kept)
    # the largest one has cells in every 16 x 16 and every 32 x 32 tile of its grid
    case, a = random_want(*BIG, G.DENSITIES[1], True, True, 3, 65536)
    rank = int(np.argmax(a.frontiers["size"]))
    member = a.label == rank
    for t in (16, 32):
        ta, tb = -(-BIG[0] // t), -(-BIG[1] // t)
        pad = np.zeros((ta * t, tb * t), bool)
        pad[:BIG[0], :BIG[1]] = member
        assert pad.reshape(ta, t, tb, t).any(axis=(1, 3)).all(), t


def test_the_constructed_grids_are_what_they_were_built_to_be():
    for name, (case, a, facts) in constructed_want().items():
        if "counts" in facts:
            assert tuple(a.counts) == facts["counts"], (name, a.counts)
        for rank, fields in facts.get("records", {}).items():
            for f, v in fields.items():
                assert int(a.frontiers[rank][f]) == v, (name, rank, f, int(a.frontiers[rank][f]))
        for at, v in facts.get("label", {}).items():
            assert int(a.label[at]) == v, (name, at)
    cw = constructed_want()
    case, a, _ = cw["serpentine"]
    assert a.counts[3] == 1 and int(a.frontiers[0]["size"]) == 2175 and (int(a.frontiers[0]["min_a"]), int(a.frontiers[0]["max_a"])) == (0, 64)
    case, a, _ = cw["diagonal_pairs"]
    assert a.counts[3] == 64 and (a.frontiers["size"] == 2).all()
    assert G.frontiers_np(*case, variant="four").counts[3] == 128
    # every tile corner of a tile edge that is a multiple of 8 (up to the grid) has a pair across it
    lab = a.label
    for i in range(1, 9):
        for j in range(1, 9):
            x, y = 8 * i, 8 * j
            d, e = (lab[x - 1, y - 1], lab[x, y]), (lab[x - 1, y], lab[x, y - 1])
            assert (d[0] == d[1] != G.NONE) != (e[0] == e[1] != G.NONE), (i, j)


def test_every_misreading_of_the_contract_changes_a_stated_case():
    case = G.misreading_case()
    right = G.frontiers_np(*case)
    assert right.counts[2:5] == (1752, 37, 7)
    got = {}
    for variant, (field, _) in MISREADINGS.items():
        wrong = G.frontiers_np(*case, variant=variant)
        if field == "label":
            got[variant] = (field, int((wrong.label != right.label).sum()))
        else:
            k = min(len(wrong.frontiers), len(right.frontiers))
            got[variant] = (field, int((wrong.frontiers[field][:k] != right.frontiers[field][:k]).sum()))
        assert got[variant][1] > 0, variant
    assert got == MISREADINGS, got
    assert set(MISREADINGS) == set(G.VARIANTS)


def _api_params(prm):
    from stereo_vo_amd import api
    return api.GridFrontierParams(*prm)


def test_pure_entries_and_refusals_without_a_context():
    from stereo_vo_amd import api
    L = api.lib()
    g = api.voxel_grid_default_params(0.1)
    cp = api.grid_clearance_default_params(g, 0.1)
    d = api.grid_frontier_default_params(cp)
    assert (d.na, d.nb, d.free_mask, d.unknown_mask, d.min_size, d.max_frontiers) == (256, 256, 1 << api.VOXEL_GRID_LEVEL, 1 << api.VOXEL_GRID_UNKNOWN, 3, 1024)
    cp.na, cp.nb = 17, 300
    d = api.grid_frontier_default_params(cp)
    assert (d.na, d.nb) == (17, 300)
    for field, value in (("na", 0), ("nb", 8193), ("na", 8192)):  # 8192 x 2049 is beyond 2^24
        bad = api.GridClearanceParams(17, 2049, 4, 64, 0.5, 0.0)
        setattr(bad, field, value)
        with pytest.raises(api.SvoError):
            api.grid_frontier_default_params(bad)
    assert L.svo_grid_frontier_default_params(None, C.byref(d)) == -1 and L.svo_grid_frontier_default_params(C.byref(cp), None) == -1
    ws = api.grid_frontier_workspace_bytes
    assert ws(0, 5, 1) == 0 and ws(5, -1, 1) == 0 and ws(5, 5, 0) == 0 and ws(5, 5, 65537) == 0 and ws(8192, 2049, 1) == 0 and ws(40000, 40000, 1) == 0
    r8 = lambda b: (b + 7) // 8 * 8
    for na, nb, mf in ((1, 1, 1), (15, 17, 64), (256, 256, 1024), (130, 300, 4096), (8192, 2048, 65536)):
        n = na * nb
        assert ws(na, nb, mf) == 256 + 64 * mf + r8(4 * -(-n // 256)) + r8(12 * n) <= 16 * n + 64 * mf + 4096 and ws(na, nb, mf) % 8 == 0
    assert api.GRID_FRONTIER_NONE == 0xFFFFFFFF and api.GRID_FRONTIER_DTYPE == G.RECORD and C.sizeof(api.GridFrontierParams) == 24
    assert len(api.GRID_FRONTIER_COUNTS) == 7
    # a null context is refused by every entry before anything else is looked at
    buf = (C.c_double * 12)()
    out = api.GridFrontierOut(C.addressof(buf))
    assert L.svo_grid_frontiers_dev(None, buf, None, None, C.byref(d), buf, C.byref(out), None) == -1
    assert L.svo_grid_frontiers(None, buf, None, None, C.byref(d), C.byref(out), None) == -1
    assert L.svo_grid_frontiers_dev(None, None, None, None, None, None, None, None) == -1
    assert L.svo_grid_frontier_set_mode(None, 1) == -1


def test_grid_frontier_args_every_refusal_the_sizes_the_geometry_and_the_defaults(tmp_path):
    """host/frontier_args.h on the CPU under ASan + UBSan: every refusal at its boundary with code and exact message, the order of the
    refusals, the workspace's size, layout and bound, the tile, seam-cell and scan-block counts at 1 x 1, T - 1, T, T + 1, 8192 x 2048
    and past 2^32, the defaults."""
    _run_sanitized(tmp_path, "grid_frontier_args_test", "grid frontier args ok")


# ===================================================================================================== GPU
_SENT = {"frontiers": (np.int64, 0x5A5A5A5A5A5A5A5A), "goal_cells": (np.int32, 0x3333CCCC), "label": (np.int32, 0x5555AAAA)}
_REC_SENT = np.full(6, 0x5A5A5A5A5A5A5A5A, np.int64).view(G.RECORD)[0]


class _Dev:
    """A case's device buffers: cls, blocked and cost between guard elements, a dirty workspace and sentinel-filled outputs with a guard
    element before and behind each.  skip: of OUTPUTS, the outputs passed as NULL."""

    def __init__(self, case, skip=(), counts=True):
        import torch
        from stereo_vo_amd import api
        self.case, self.prm, self.skip, self.counts = case, case.prm, tuple(skip), counts
        n, mf = self.prm.na * self.prm.nb, self.prm.max_frontiers
        self.n, self.mf = n, mf

        def guarded(a, t, guard):
            d = torch.full((len(a) + 2,), guard, dtype=t, device="cuda")
            d[1:-1] = torch.from_numpy(np.ascontiguousarray(a)).cuda()
            return d

        # a guard read as a cell would be UNKNOWN, passable and cheap
        self.cls = guarded(case.cls.ravel(), torch.uint8, G.UNKNOWN)
        self.blocked = None if case.blocked is None else guarded(case.blocked.ravel(), torch.uint8, 0)
        self.cost = None if case.cost is None else guarded(case.cost.ravel().view(np.int32), torch.int32, 0)
        words = api.grid_frontier_workspace_bytes(self.prm.na, self.prm.nb, mf) // 8
        self.ws = torch.full((words + 2,), 0x7F7F7F7F7F7F7F7F, dtype=torch.int64, device="cuda")
        sizes = {"frontiers": 6 * mf, "goal_cells": mf, "label": n}
        self.bufs = {k: torch.full((sizes[k] + 2,), v, dtype=getattr(torch, np.dtype(t).name), device="cuda") for k, (t, v) in _SENT.items()}
        self.cnt = torch.full((10,), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()

    def call(self, ctx, **over):
        p = _api_params(self.prm._replace(**over))
        ptr = {k: None if k in self.skip else b.data_ptr() + b.element_size() for k, b in self.bufs.items()}
        out = ctx.grid_frontiers(self.cls.data_ptr() + 1, p, blocked_ptr=None if self.blocked is None else self.blocked.data_ptr() + 1,
                                 cost_ptr=None if self.cost is None else self.cost.data_ptr() + 4, workspace_ptr=self.ws.data_ptr() + 8,
                                 counts_ptr=self.cnt.data_ptr() + 8 if self.counts else None, **{k + "_ptr": v for k, v in ptr.items()})
        assert out["label"] == ptr["label"] and (out["na"], out["nb"], out["max_frontiers"]) == (self.prm.na, self.prm.nb, self.mf)
        ctx.sync()

    def read(self, keep=None):
        """{"frontiers": all max_frontiers records, "goal_cells", "label", "counts": the eight}, None for what was skipped"""
        case, prm = self.case, self.prm
        w = self.ws.cpu().numpy()
        assert w[0] == w[-1] == 0x7F7F7F7F7F7F7F7F
        assert np.array_equal(self.cls.cpu().numpy()[1:-1].reshape(case.cls.shape), case.cls)  # only read
        if self.blocked is not None:
            assert np.array_equal(self.blocked.cpu().numpy()[1:-1].reshape(case.cls.shape), case.blocked)
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
        if got["frontiers"] is not None:
            got["frontiers"] = got["frontiers"].view(G.RECORD)
        if got["goal_cells"] is not None:
            got["goal_cells"] = got["goal_cells"].view(np.uint32)
        if got["label"] is not None:
            got["label"] = got["label"].view(np.uint32).reshape(prm.na, prm.nb)
        return got


def _eq(got, w, what=""):
    nw = w.counts[5]
    assert nw == len(w.frontiers)
    if got["counts"] is not None:
        assert got["counts"] == tuple(w.counts) + (0,), (what, got["counts"], w.counts)
    if got["frontiers"] is not None:
        rec = got["frontiers"]
        bad = [i for i in range(nw) if rec[i] != w.frontiers[i]]
        assert not bad, (what, "records", bad[:4], rec[bad[0]], w.frontiers[bad[0]])
        assert (rec[nw:] == _REC_SENT).all(), (what, "records past n_written")
    if got["goal_cells"] is not None:
        assert np.array_equal(got["goal_cells"], w.goal_cells), (what, "goal_cells", int((got["goal_cells"] != w.goal_cells).sum()))
    if got["label"] is not None:
        assert np.array_equal(got["label"], w.label), (what, "label", int((got["label"] != w.label).sum()))


def _run(ctx, case, how="dev", skip=(), counts=True, keep=None):
    if how == "host":
        from stereo_vo_amd import api
        r = ctx.grid_frontiers_host(case.cls, case.blocked, case.cost, _api_params(case.prm))
        rec = np.full(case.prm.max_frontiers, _REC_SENT, G.RECORD)
        rec[:len(r["frontiers"])] = r["frontiers"]
        assert tuple(r["counts"]) == api.GRID_FRONTIER_COUNTS and len(r["frontiers"]) == r["counts"]["n_written"]
        return {"frontiers": rec, "goal_cells": r["goal_cells"], "label": r["label"], "counts": tuple(r["counts"].values()) + (0,)}
    d = _Dev(case, skip, counts)
    d.call(ctx)
    return d.read(keep)


@pytest.mark.gpu
@pytest.mark.parametrize("na,nb", G.SIZES)
def test_random_grids(ctx, na, nb):
    for density in G.DENSITIES:
        for b in (False, True):
            for c in (False, True):
                case, w = random_want(na, nb, density, b, c)
                got = _run(ctx, case)
                print(na, nb, density, b, c, "counts", got["counts"])
                _eq(got, w, (density, b, c))


@pytest.mark.gpu
def test_constructed_grids_through_both_entries(ctx):
    for name, (case, w, facts) in constructed_want().items():
        if "counts" in facts:
            assert tuple(w.counts) == facts["counts"], name
        for how in ("dev", "host"):
            got = _run(ctx, case, how)
            print(name, how, got["counts"])
            _eq(got, w, (name, how))


@pytest.mark.gpu
def test_max_frontiers_1_64_and_4096_truncate_the_records_not_the_labels(ctx):
    seen = set()
    for density, mf in TRUNCATED:
        case, w = random_want(*BIG, density, True, True, 3, mf)
        full = random_want(*BIG, density, True, True, 3, 65536)[1]
        n_kept = w.counts[4]
        assert w.counts[5] == min(n_kept, mf) and np.array_equal(w.label, full.label) and int(w.label[w.label != G.NONE].max()) == n_kept - 1
        assert (w.goal_cells[w.counts[5]:] == G.NONE).all() and w.frontiers.tobytes() == full.frontiers[:w.counts[5]].tobytes()
        seen.add("cut" if n_kept > mf else "whole")
        got = _run(ctx, case)
        print(density, mf, got["counts"])
        _eq(got, w, (density, mf))
        _eq(_run(ctx, case, "host"), w, (density, mf, "host"))
    assert seen == {"cut", "whole"}


@pytest.mark.gpu
def test_min_size_1_and_2_to_the_24(ctx):
    for ms in MIN_SIZES:
        case, w = random_want(63, 65, G.DENSITIES[1], True, True, ms)
        assert (w.counts[4] == w.counts[3] > 7) if ms == 1 else (w.counts[4] == 0 and (w.label == G.NONE).all() and (w.goal_cells == G.NONE).all())
        _eq(_run(ctx, case), w, ms)
        _eq(_run(ctx, case, "host"), w, (ms, "host"))


@pytest.mark.gpu
def test_optional_outputs_the_host_entry_a_repeated_call_and_the_plain_mode(ctx):
    from stereo_vo_amd import api
    case, w = random_want(63, 65, G.DENSITIES[0], True, True, 3, 64)
    assert w.counts[4] > 64  # truncated: records past the written ones exist in neither entry
    for skip in [(k,) for k in OUTPUTS] + [("frontiers", "goal_cells"), ("frontiers", "label"), ("goal_cells", "label")]:
        got = _run(ctx, case, skip=skip)
        assert all((got[k] is None) == (k in skip) for k in OUTPUTS)
        _eq(got, w, skip)
    _eq(_run(ctx, case, counts=False), w, "no counts")
    _eq(_run(ctx, case, skip=("frontiers", "label"), counts=False), w, "goal_cells alone")
    # the host entry: keywords instead of a parameter set; the caller's records past n_written come back as they were
    case2, w2 = random_want(63, 65, G.DENSITIES[1], True, True)
    r = ctx.grid_frontiers_host(case2.cls, blocked=case2.blocked, cost=case2.cost)
    assert r["frontiers"].tobytes() == w2.frontiers.tobytes() and np.array_equal(r["label"], w2.label) and tuple(r["counts"].values()) == tuple(w2.counts)
    rec = np.full(case2.prm.max_frontiers, _REC_SENT, G.RECORD)
    p = _api_params(case2.prm)
    assert ctx.L.svo_grid_frontiers(ctx.h, case2.cls.ctypes.data, case2.blocked.ctypes.data, case2.cost.ctypes.data, C.byref(p),
                                    C.byref(api.GridFrontierOut(rec.ctypes.data, None, None)), None) == 0
    nw = w2.counts[5]
    assert 0 < nw < len(rec) and rec[:nw].tobytes() == w2.frontiers.tobytes() and (rec[nw:] == _REC_SENT).all()
    # twice: the same bytes in every output; once more without the combining of runs: the same bytes again
    first, second, plain = {}, {}, {}
    big, wb = random_want(*BIG, G.DENSITIES[1], True, True)
    _eq(_run(ctx, big, keep=first), wb)
    _eq(_run(ctx, big, keep=second), wb)
    ctx.grid_frontier_set_mode(False)
    try:
        _eq(_run(ctx, big, keep=plain), wb, "plain")
    finally:
        ctx.grid_frontier_set_mode(None)
    assert first == second == plain and set(first) == set(_SENT)


@pytest.mark.gpu
def test_bad_calls_launch_nothing_and_leave_the_context_usable(ctx):
    from stereo_vo_amd import api
    L = ctx.L
    case, w = random_want(63, 65, G.DENSITIES[1], True, True)
    good = case.prm
    d = _Dev(case)
    O = api.GridFrontierOut
    P = {k: b.data_ptr() + b.element_size() for k, b in d.bufs.items()}
    full = lambda **kw: O(**{**P, **kw})
    A = dict(cls=d.cls.data_ptr() + 1, blocked=d.blocked.data_ptr() + 1, cost=d.cost.data_ptr() + 4, ws=d.ws.data_ptr() + 8, counts=d.cnt.data_ptr() + 8)

    def dev(prm=good, out=None, null_prm=False, null_out=False, **kw):
        a = {**A, **kw}
        o = out if out is not None else full()
        p = _api_params(prm)
        return L.svo_grid_frontiers_dev(ctx.h, a["cls"], a["blocked"], a["cost"], None if null_prm else C.byref(p), a["ws"],
                                        None if null_out else C.byref(o), a["counts"])

    r = good._replace
    hlabel = np.full((good.na, good.nb), 0x5555AAAA, np.uint32)

    def host(prm=good, cls=case.cls.ctypes.data, out=None, null_out=False, null_prm=False):
        o = out if out is not None else O(None, None, hlabel.ctypes.data)
        return L.svo_grid_frontiers(ctx.h, cls, None, None, None if null_prm else C.byref(_api_params(prm)), None if null_out else C.byref(o), None)

    calls = [(lambda: dev(cls=None), "null cls"), (lambda: dev(null_prm=True), "null params"), (lambda: dev(ws=None), "null workspace"),
             (lambda: dev(null_out=True), "null out"),
             (lambda: dev(r(na=0), ws=None), "null workspace"),  # the nulls before the ranges
             (lambda: dev(r(na=0)), "na outside"), (lambda: dev(r(na=8193)), "na outside"), (lambda: dev(r(nb=0)), "nb outside"),
             (lambda: dev(r(nb=8193)), "nb outside"), (lambda: dev(r(na=8192, nb=2049)), "na * nb"),
             (lambda: dev(r(free_mask=0)), "free_mask is 0"), (lambda: dev(r(unknown_mask=0)), "unknown_mask is 0"),
             (lambda: dev(r(min_size=0)), "min_size"), (lambda: dev(r(min_size=(1 << 24) + 1)), "min_size"),
             (lambda: dev(r(max_frontiers=0)), "max_frontiers"), (lambda: dev(r(max_frontiers=65537)), "max_frontiers"),
             (lambda: dev(r(free_mask=3)), "share a bit"), (lambda: dev(r(free_mask=6, unknown_mask=5)), "share a bit"),
             (lambda: dev(out=O(None, None, None)), "all null"),
             (lambda: dev(cost=A["cost"] + 2), "cost must be 4-byte"), (lambda: dev(out=full(label=P["label"] + 1)), "label must be 4-byte"),
             (lambda: dev(out=full(goal_cells=P["goal_cells"] + 2)), "goal_cells must be 4-byte"),
             (lambda: dev(out=full(frontiers=P["frontiers"] + 4)), "frontiers must be 8-byte"),
             (lambda: dev(ws=A["ws"] + 4), "workspace must be 8-byte"), (lambda: dev(counts=A["counts"] + 4), "counts must be 8-byte"),
             (lambda: dev(cost=A["cost"] + 2, counts=A["counts"] + 4), "cost must be 4-byte"),  # the 4-byte ones first
             (lambda: host(cls=None), "null cls"), (lambda: host(null_prm=True), "null params"), (lambda: host(null_out=True), "null out"),
             (lambda: host(r(min_size=0)), "min_size"), (lambda: host(r(free_mask=1)), "share a bit"), (lambda: host(out=O(None, None, None)), "all null")]
    ctx.profile_select("grid_frontier")
    for call, word in calls:
        assert call() == -1 and word in L.svo_last_error(ctx.h).decode(), (word, L.svo_last_error(ctx.h).decode())
    assert ctx.profile_read()[1] == 0
    ctx.sync()
    for k, (t, v) in _SENT.items():
        assert (d.bufs[k].cpu().numpy() == v).all(), k
    assert (d.ws.cpu().numpy() == 0x7F7F7F7F7F7F7F7F).all() and (d.cnt.cpu().numpy() == -1).all() and (hlabel == 0x5555AAAA).all()
    # the boundaries' accepted sides in one call: one bracket
    assert dev(r(min_size=1 << 24, max_frontiers=1, free_mask=0x80000002, unknown_mask=1), blocked=None, cost=None, counts=None,
               out=full(frontiers=None, label=None)) == 0
    assert ctx.profile_read()[1] == 1
    ctx.profile_select(None)
    with pytest.raises(api.SvoError):
        ctx.grid_frontiers(A["cls"], _api_params(good), label_ptr=P["label"])  # no workspace
    with pytest.raises(api.SvoError):
        ctx.grid_frontiers_host(case.cls, min_size=0)
    with pytest.raises(api.SvoError):
        ctx.grid_frontiers_host(case.cls, max_frontiers=0)
    with pytest.raises(ValueError):
        ctx.grid_frontiers_host(case.cls, params=_api_params(good._replace(na=5)))
    with pytest.raises(ValueError):
        ctx.grid_frontiers_host(case.cls, blocked=case.blocked[:5])
    # the context is what it was, and gives the frontiers
    _eq(_run(ctx, case), w)
    _eq(_run(ctx, case, "host"), w)
