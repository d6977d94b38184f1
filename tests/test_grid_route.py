"""The ground plan route (include/svo.h, "Ground plan route") against its restatement tests/grid_route_ref.py, with == on
cost, next, path up to the written length, path_len, path_status and the counts; rounds_run is only bounded.

CPU: the restatement's two routes (Dijkstra, whole-array Bellman-Ford) agree on every case used below; open unweighted grids follow
the closed form 80 max + 32 min; the constructed grids are what they were built to be; each deliberate misreading of the contract
changes a result; the not-converged grid is as far from its goal as the GPU test needs for both tile edges; the pure entries and the
refusals that need no context; stereo_vo_amd/host/route_args.h walked by tests/sanitize/grid_route_args_test.cpp under ASan + UBSan.
GPU: seeded grids of fourteen shapes at three densities with and without dist2; the constructed grids; paths at and one below their
length, every start status, 4096 starts; one round that cannot converge and the resumed calls that do; every optional output left
out; the host entry; a repeated call; bad calls.  Every device call runs into a dirty workspace and sentinel-filled outputs whose
guard elements stay, with blocked and dist2 between guard elements.

ROUNDS.  A cell whose cheapest route has h moves is final after round h (induction over h: the tile that lowered the route's next
cell wakes every tile that sees it, itself included when its sweep bound cut it short), and one more round finds nothing to do; so
max_rounds = h_max + 2 always converges.  The random and constructed cases run with that bound, taken from the restatement.

Misreadings, cells that change on the restatement (grid "mixed": 63 x 65, density 0.25, dist2 0 .. 40 with a fifth NONE, near_r2 16,
near_weight 3, one goal of three on an impassable cell, max_cost 4,011, the cost of the cell at the upper quartile; 2,306 cells reached):
  corner cutting 2,859 cost; the penalty of the cell left 2,072 cost; diagonal weight 5 2,622 cost; four neighbours 2,274 cost; the tie
  to the largest k 206 next; < max_cost 3 cost; a goal on an impassable cell used 1 cost; NONE read as near 2,285 cost; the start's
  own step paid 2,306 cost.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import grid_route_ref as G
from test_host_sanitizers import _run_sanitized

MISREADINGS = {"corner_cut": ("cost", 2859), "pen_left": ("cost", 2072), "diag5": ("cost", 2622), "four": ("cost", 2274),
               "tie_largest": ("next", 206), "lt_max": ("cost", 3), "goal_blocked": ("cost", 1), "none_near": ("cost", 2285),
               "start_step": ("cost", 2306)}
OUTPUTS = ("next", "path")


def _freeze(r):
    for a in r[:5]:
        a.setflags(write=False)
    return r


def _bounded(case):
    """(the case with max_rounds set to the bound of the docstring, its restatement)"""
    w = G.route_np(case.blocked, case.dist2, case.prm, case.goals, case.starts)
    reached = np.flatnonzero(w.cost.ravel() != G.NONE)
    hops = G.route_np(case.blocked, case.dist2, case.prm._replace(max_path=1), case.goals, reached).path_len
    rounds = int(hops.max()) + 1 if len(reached) else 2  # path_len = moves + 1
    assert rounds <= 4096, rounds
    return case._replace(prm=case.prm._replace(max_rounds=rounds)), _freeze(w)


@functools.lru_cache(maxsize=None)
def random_want(na, nb, density, with_dist2):
    return _bounded(G.random_case(na, nb, density, with_dist2))


@functools.lru_cache(maxsize=None)
def constructed_want():
    return {name: _bounded(case) + (facts,) for name, (case, facts) in G.constructed().items()}


RANDOM = [(na, nb, density, d2) for na, nb in G.SIZES for density in G.DENSITIES for d2 in (False, True)]


# ===================================================================================================== CPU
def test_the_two_routes_of_the_restatement_agree_on_every_case():
    reached = unreached = truncated = 0
    for na, nb, density, d2 in RANDOM:
        case, a = random_want(na, nb, density, d2)
        assert G.same(a, G.route_py(case.blocked, case.dist2, case.prm, case.goals, case.starts)), (na, nb, density, d2)
        assert sum(a.counts[1:4]) == na * nb and a.counts[3] == int((case.blocked != 0).sum())
        reached += a.counts[1]
        unreached += a.counts[2]
        truncated += int((a.path_status == G.TRUNCATED).sum())
    # the cases are what the kernels' paths need: reached and cut-off cells, paths longer than max_path, several tiles and rounds
    assert reached > 50000 and unreached > 1000 and truncated >= 3
    assert random_want(130, 300, 0.25, True)[0].prm.max_rounds > 100
    for name, (case, a, _) in constructed_want().items():
        assert G.same(a, G.route_py(case.blocked, case.dist2, case.prm, case.goals, case.starts)), name
    case = G.misreading_case()
    assert G.same(G.route_np(*case), G.route_py(*case))
    case = G.not_converged_case()
    assert G.same(G.route_np(*case), G.route_py(*case))


def test_open_unweighted_grids_follow_the_closed_form():
    """With no obstacle and no penalty a route of da rows and db columns takes min(da, db) diagonals (7 * 16 = 112 each, against 160 for
    the two axis moves it replaces) and max - min axis moves (5 * 16 = 80): 112 min + 80 (max - min) = 80 max + 32 min, the 5-7
    chamfer distance 5 max + 2 min times 16."""
    for na, nb, goal in ((1, 1, (0, 0)), (7, 40, (3, 11)), (33, 35, (32, 0)), (40, 40, (0, 0))):
        b = np.zeros((na, nb), np.uint8)
        got = G.route_np(b, None, G.params(b), [goal[0] * nb + goal[1]])
        da, db = np.abs(np.arange(na) - goal[0])[:, None], np.abs(np.arange(nb) - goal[1])[None, :]
        assert np.array_equal(got.cost, 80 * np.maximum(da, db) + 32 * np.minimum(da, db)), (na, nb)
        assert G.open_cost(3, 5) == 5 * 80 + 3 * 32 == 2 * 80 + 3 * 112


def test_the_constructed_grids_are_what_they_were_built_to_be():
    for name, (case, a, facts) in constructed_want().items():
        if "counts" in facts:
            assert a.counts == facts["counts"], (name, a.counts)
        for at, value in facts.get("cost", {}).items():
            assert int(a.cost[at]) == value, (name, at, int(a.cost[at]))
        for at, k in facts.get("next", {}).items():
            assert int(a.next[at]) == k, (name, at, int(a.next[at]))
    cw = constructed_want()
    case, a, _ = cw["wall_gap"]
    assert 7 * 9 + 4 in a.path[0, :a.path_len[0]] and a.path_status[0] == G.OK and a.path[0, a.path_len[0] - 1] == 0
    case, a, _ = cw["penalty_corridor"]
    assert not set(a.path[0, :a.path_len[0]].tolist()) & {2 * 9 + c for c in range(2, 7)} and a.path_len[0] == 9
    straight = G.route_np(case.blocked, None, case.prm, case.goals, case.starts)
    assert straight.cost[2, 8] == 640 < a.cost[2, 8] < 3 * 80 + 5 * 5 * (16 + 1600)  # longer than the straight way, cheaper than paying for it
    case, a, _ = cw["dist2_none"]
    assert (case.dist2 == G.NONE).sum() > 50 and a.counts[1] > 200
    case, a, _ = cw["squeezed"]
    assert a.path_status[0] == G.UNREACHED and a.path_len[0] == 0
    case, a, _ = cw["exact_max_cost"]
    assert list(a.path_status) == [G.OK, G.UNREACHED] and list(a.path_len) == [4, 0]


def test_every_misreading_of_the_contract_changes_a_result():
    case = G.misreading_case()
    right = G.route_np(*case)
    assert (right.cost == case.prm.max_cost).sum() >= 1 and right.counts[0] == 2 and right.counts[2] > 500
    got = {}
    for variant, (field, _) in MISREADINGS.items():
        wrong = G.route_np(*case, variant=variant)
        got[variant] = (field, int((getattr(right, field) != getattr(wrong, field)).sum()))
        assert got[variant][1] > 0, variant
    assert got == MISREADINGS, got
    assert set(MISREADINGS) == set(G.VARIANTS)


def test_the_not_converged_grid_is_farther_than_three_tiles_for_both_tile_edges():
    case = G.not_converged_case()
    w = G.route_np(*case)
    assert w.counts == (1, 8000, 0, 0, 1) and w.cost[39, 199] == G.open_cost(39, 199)
    for t in G.TILES:
        # round 1 runs the tiles (0..1, 0..1); what they can lower lies in tile rows and columns 0..1, so a cell of tile column >= 3
        # (three or more tiles from the goal's) has no cost after one round, and there are such cells
        assert 199 // t >= 3 and (w.cost[:, 3 * t:] != G.NONE).all()


def _api_params(prm):
    from stereo_vo_amd import api
    return api.GridRouteParams(*prm)


def test_pure_entries_and_refusals_without_a_context():
    from stereo_vo_amd import api
    L = api.lib()
    g = api.voxel_grid_default_params(0.1)
    cp = api.grid_clearance_default_params(g, 0.1)
    d = api.grid_route_default_params(cp)
    assert (d.na, d.nb, d.near_r2, d.near_weight, d.max_cost, d.max_rounds, d.max_path, d.resume) == (256, 256, 0, 0, 0x7F000000, 64, 4096, 0)
    cp.na, cp.nb = 17, 300
    d = api.grid_route_default_params(cp)
    assert (d.na, d.nb) == (17, 300)
    for field, value in (("na", 0), ("nb", 8193), ("na", 8192)):  # 8192 x 2049 is beyond 2^24
        bad = api.GridClearanceParams(17, 2049, 4, 64, 0.5, 0.0)
        setattr(bad, field, value)
        with pytest.raises(api.SvoError):
            api.grid_route_default_params(bad)
    assert L.svo_grid_route_default_params(None, C.byref(d)) == -1 and L.svo_grid_route_default_params(C.byref(cp), None) == -1
    ws = api.grid_route_workspace_bytes
    assert ws(0, 5) == 0 and ws(5, -1) == 0 and ws(1, 1) % 8 == 0 and ws(1, 1) >= 64 + 8 + 1
    # a header, two words per tile (whatever the tile's edge, between 16 and 32) and a byte per cell
    for na, nb in ((256, 256), (130, 300), (8192, 2048)):
        tiles = [-(-na // t) * -(-nb // t) for t in G.TILES]
        assert ws(na, nb) % 8 == 0 and 64 + 8 * min(tiles) + na * nb <= ws(na, nb) <= 64 + 8 * max(tiles) + na * nb + 7
    assert ws(40000, 40000) > 40000 * 40000  # past 2^32
    assert (api.GRID_ROUTE_NONE, api.GRID_ROUTE_MAX_COST, api.GRID_ROUTE_NOT_CONVERGED) == (0xFFFFFFFF, 0x7F000000, 4)
    # a null context is refused by both entries before anything else is looked at
    buf = (C.c_double * 12)()
    out = api.GridRouteOut(C.addressof(buf))
    assert L.svo_grid_route_dev(None, buf, None, C.byref(d), buf, 1, None, 0, buf, C.byref(out), None) == -1
    assert L.svo_grid_route(None, buf, None, C.byref(d), buf, 1, None, 0, C.byref(out), None) == -1
    assert L.svo_grid_route_dev(None, None, None, None, None, 0, None, 0, None, None, None) == -1


def test_grid_route_args_every_refusal_the_sizes_the_geometry_and_the_defaults(tmp_path):
    """host/route_args.h on the CPU under ASan + UBSan: every refusal at its boundary with code and exact message, the order of the
    refusals, the workspace size and layout, the tile count and launch geometry at 1 x 1, T - 1, T, T + 1, 8192 x 2048 and past 2^32,
    the defaults."""
    _run_sanitized(tmp_path, "grid_route_args_test", "grid route args ok")


# ===================================================================================================== GPU
_SENT = {"cost": (np.int32, 0x5555AAAA), "next": (np.uint8, 0xBB), "path": (np.int32, 0x3333CCCC), "path_len": (np.int32, 0x77777777),
         "path_status": (np.uint8, 0xEE)}
_GROUP = {"next": ("next",), "path": ("path", "path_len", "path_status")}


class _Dev:
    """A case's device buffers: blocked, dist2, goals and starts between guard elements, a dirty workspace and sentinel-filled outputs
    with a guard element before and behind each.  skip: of OUTPUTS, the outputs passed as NULL."""

    def __init__(self, case, skip=(), counts=True):
        import torch
        from stereo_vo_amd import api
        self.case, self.prm, self.skip, self.counts = case, case.prm, tuple(skip), counts
        n, ns = self.prm.na * self.prm.nb, len(case.starts)
        self.n, self.ns = n, ns

        def guarded(a, t, guard):
            d = torch.full((len(a) + 2,), guard, dtype=t, device="cuda")
            if len(a):
                d[1:-1] = torch.from_numpy(np.ascontiguousarray(a)).cuda()
            return d

        self.blocked = guarded(case.blocked.ravel(), torch.uint8, 0)  # a guard read as a cell would be passable, and near
        self.dist2 = None if case.dist2 is None else guarded(case.dist2.ravel().view(np.int32), torch.int32, 0)
        self.goals = guarded(np.asarray(case.goals, np.uint32).view(np.int32), torch.int32, 0)
        self.starts = guarded(np.asarray(case.starts, np.uint32).view(np.int32), torch.int32, 0)
        words = api.grid_route_workspace_bytes(self.prm.na, self.prm.nb) // 8
        self.ws = torch.full((words + 2,), 0x7F7F7F7F7F7F7F7F, dtype=torch.int64, device="cuda")
        sizes = {"cost": n, "next": n, "path": ns * self.prm.max_path, "path_len": ns, "path_status": ns}
        self.bufs = {k: torch.full((sizes[k] + 2,), v, dtype=getattr(torch, np.dtype(t).name), device="cuda") for k, (t, v) in _SENT.items()}
        self.cnt = torch.full((10,), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()

    def call(self, ctx, **over):
        p = _api_params(self.prm._replace(**over))
        ptr = {k: b.data_ptr() + b.element_size() for k, b in self.bufs.items()}
        for group in self.skip:
            for k in _GROUP[group]:
                ptr[k] = None
        if not self.ns:
            ptr["path"] = ptr["path_len"] = ptr["path_status"] = None
        out = ctx.grid_route(self.blocked.data_ptr() + 1, p, self.goals.data_ptr() + 4, len(self.case.goals), workspace_ptr=self.ws.data_ptr() + 8,
                             dist2_ptr=None if self.dist2 is None else self.dist2.data_ptr() + 4,
                             starts_ptr=self.starts.data_ptr() + 4 if self.ns else None, n_starts=self.ns,
                             counts_ptr=self.cnt.data_ptr() + 8 if self.counts else None, **{k + "_ptr": v for k, v in ptr.items()})
        assert out["cost"] == ptr["cost"] and (out["na"], out["nb"]) == (self.prm.na, self.prm.nb)
        ctx.sync()

    def read(self, keep=None):
        """A G.Route with None for what was skipped; path rows keep their sentinel where nothing was written."""
        case, prm = self.case, self.prm
        w = self.ws.cpu().numpy()
        assert w[0] == w[-1] == 0x7F7F7F7F7F7F7F7F
        assert np.array_equal(self.blocked.cpu().numpy()[1:-1].reshape(case.blocked.shape), case.blocked)  # only read
        if self.dist2 is not None:
            assert np.array_equal(self.dist2.cpu().numpy()[1:-1].view(np.uint32).reshape(case.dist2.shape), case.dist2)
        got = {}
        absent = {k for group in self.skip for k in _GROUP[group]} | (set(_GROUP["path"]) if not self.ns else set())
        for k, (t, v) in _SENT.items():
            a = self.bufs[k].cpu().numpy()
            assert a[0] == v and a[-1] == v, k  # nothing beside the outputs is written
            if k in absent:
                assert (a == v).all(), k
                got[k] = None
            else:
                got[k] = a[1:-1]
            if keep is not None:
                keep[k] = a.tobytes()
        c = self.cnt.cpu().numpy()
        assert c[0] == c[-1] == -1 and (self.counts or (c == -1).all())
        if self.counts:
            assert c[7] == 0 and c[8] == 0
        u32 = lambda a: None if a is None else a.view(np.uint32)
        shape = (prm.na, prm.nb)
        return G.Route(u32(got["cost"]).reshape(shape), None if got["next"] is None else got["next"].reshape(shape),
                       None if got["path"] is None else u32(got["path"]).reshape(self.ns, prm.max_path), u32(got["path_len"]), got["path_status"],
                       tuple(int(v) for v in c[1:7]) if self.counts else None)


def _eq(got, w, prm, what=""):
    assert np.array_equal(got.cost, w.cost), (what, "cost", int((got.cost != w.cost).sum()))
    if got.next is not None:
        assert np.array_equal(got.next, w.next), (what, "next", int((got.next != w.next).sum()))
    if got.path is not None:
        assert np.array_equal(got.path_len, w.path_len), (what, "path_len", got.path_len[:8], w.path_len[:8])
        assert np.array_equal(got.path_status, w.path_status), (what, "path_status")
        written = np.arange(got.path.shape[1])[None, :] < np.minimum(w.path_len, got.path.shape[1])[:, None]
        assert np.array_equal(got.path[written], w.path[written]), (what, "path")
        assert (got.path[~written] == 0x3333CCCC).all(), (what, "cells past the written ones")
    if got.counts is not None:
        assert tuple(got.counts[:5]) == tuple(w.counts), (what, got.counts, w.counts)
        assert 0 <= got.counts[5] <= prm.max_rounds, (what, got.counts)


def _run(ctx, case, how="dev", skip=(), counts=True, keep=None):
    if how == "host":
        r = ctx.grid_route_host(case.blocked, case.goals, case.dist2, case.starts if len(case.starts) else None, _api_params(case.prm))
        c = r["counts"]
        path = r.get("path")
        if path is not None:  # the host wrapper fills with NONE what the device tests fill with their sentinel
            written = np.arange(path.shape[1])[None, :] < np.minimum(r["path_len"], path.shape[1])[:, None]
            path = np.where(written, path, 0x3333CCCC).astype(np.uint32)
        return G.Route(r["cost"], r["next"], path, r.get("path_len"), r.get("path_status"),
                       tuple(c[k] for k in ("n_goals_used", "n_reached", "n_unreached", "n_impassable", "converged", "rounds_run")))
    d = _Dev(case, skip, counts)
    d.call(ctx)
    return d.read(keep)


@pytest.mark.gpu
@pytest.mark.parametrize("na,nb", G.SIZES)
def test_random_grids(ctx, na, nb):
    for density in G.DENSITIES:
        for d2 in (False, True):
            case, w = random_want(na, nb, density, d2)
            got = _run(ctx, case)
            print(na, nb, density, d2, "max_rounds", case.prm.max_rounds, "counts", got.counts)
            _eq(got, w, case.prm, (density, d2))


@pytest.mark.gpu
def test_constructed_grids(ctx):
    for name, (case, w, facts) in constructed_want().items():
        if "counts" in facts:
            assert w.counts == facts["counts"], name
        for how in ("dev", "host"):
            got = _run(ctx, case, how)
            print(name, how, got.counts)
            _eq(got, w, case.prm, (name, how))


@pytest.mark.gpu
def test_paths_every_status_the_length_and_one_less_and_4096_starts(ctx):
    case, w, _ = constructed_want()["wall_gap"]
    b = case.blocked
    full = int(w.path_len[0])
    assert full >= 10
    # a start on the goal, a blocked start, the far corner, an out-of-grid start
    starts = np.array([0, 4, 8, 81, 0xFFFFFFFF, 7 * 9 + 4], np.uint32)
    for max_path in (full, full - 1, 1):
        c = case._replace(starts=starts, prm=case.prm._replace(max_path=max_path))
        ww = G.route_np(*c)
        assert list(ww.path_status) == [G.OK, G.UNREACHED, G.TRUNCATED if max_path < full else G.OK, G.OUT_OF_GRID, G.OUT_OF_GRID,
                                        G.TRUNCATED if max_path == 1 else G.OK]
        assert list(ww.path_len) == [1, 0, full, 0, 0, int(ww.path_len[5])]
        _eq(_run(ctx, c), ww, c.prm, max_path)
        _eq(_run(ctx, c, "host"), ww, c.prm, (max_path, "host"))
    # an unreached start that is passable
    sq, wq, _ = constructed_want()["squeezed"]
    assert wq.path_status[0] == G.UNREACHED and sq.blocked.ravel()[sq.starts[0]] == 0
    _eq(_run(ctx, sq), wq, sq.prm, "squeezed")
    # 4096 starts over a random grid, 64 cells each
    rc, _ = random_want(63, 65, 0.25, True)
    rng = np.random.default_rng(5)
    c = rc._replace(starts=rng.integers(0, 63 * 65 + 20, 4096).astype(np.uint32), prm=rc.prm._replace(max_path=48))
    ww = G.route_np(*c)
    assert {G.OK, G.TRUNCATED, G.UNREACHED, G.OUT_OF_GRID} == set(ww.path_status.tolist())
    _eq(_run(ctx, c), ww, c.prm, "4096 starts")


@pytest.mark.gpu
def test_one_round_cannot_converge_and_resumed_calls_do(ctx):
    case = G.not_converged_case()
    w = G.route_np(*case)
    d = _Dev(case)
    d.call(ctx)
    got = d.read()
    assert got.counts[:5] == (1, 0, 0, 0, 0) and got.counts[5] == 1, got.counts
    assert (got.next == 0xBB).all() and (got.path == 0x3333CCCC).all()  # not written
    assert (got.path_len == 0).all() and (got.path_status == G.NOT_CONVERGED).all()
    for t in G.TILES:
        assert (got.cost[:, 3 * t:] == G.NONE).all()
    some = got.cost != G.NONE
    assert some.sum() >= 16 * 16 and (got.cost[some] >= w.cost[some]).all() and got.cost[0, 0] == 0
    calls = 0
    while got.counts[4] == 0 and calls < 64:
        d.call(ctx, resume=1)
        got = d.read()
        calls += 1
        some = got.cost != G.NONE
        assert (got.cost[some] >= w.cost[some]).all()
    print("resumed calls", calls)
    assert got.counts[4] == 1 and 2 <= calls
    _eq(got, w, case.prm, "resumed")
    # a further resumed call finds nothing to do and gives the same again; with more rounds per call it resumes as well
    d.call(ctx, resume=1, max_rounds=3)
    got = d.read()
    assert got.counts[5] == 0
    _eq(got, w, case.prm._replace(max_rounds=3), "after convergence")
    d = _Dev(case)
    d.call(ctx, max_rounds=2)
    assert d.read().counts[4] == 0
    d.call(ctx, resume=1, max_rounds=63)
    _eq(d.read(), w, case.prm._replace(max_rounds=63), "2 + 63 rounds")


@pytest.mark.gpu
def test_optional_outputs_the_host_entry_and_a_repeated_call(ctx):
    from stereo_vo_amd import api
    case, w = random_want(63, 65, 0.25, True)
    for skip in [(k,) for k in OUTPUTS] + [OUTPUTS]:
        got = _run(ctx, case, skip=skip)
        assert (got.next is None) == ("next" in skip) and (got.path is None) == ("path" in skip)
        _eq(got, w, case.prm, skip)
    _eq(_run(ctx, case, counts=False), w, case.prm, "no counts")
    _eq(_run(ctx, case, skip=OUTPUTS, counts=False), w, case.prm, "cost alone")
    nostarts = case._replace(starts=np.zeros(0, np.uint32))
    _eq(_run(ctx, nostarts), w, case.prm, "no starts")
    # the host entry: everything, keywords instead of a parameter set, cost alone
    _eq(_run(ctx, case, "host"), w, case.prm, "host")
    r = ctx.grid_route_host(case.blocked, case.goals, dist2=case.dist2, near_r2=16, near_weight=3, max_rounds=case.prm.max_rounds)
    assert np.array_equal(r["cost"], w.cost) and np.array_equal(r["next"], w.next) and "path" not in r
    assert tuple(r["counts"].values())[:5] == w.counts
    cost = np.full(case.blocked.shape, 0x5555AAAA, np.uint32)
    goals = np.asarray(case.goals, np.uint32)
    p = _api_params(case.prm)
    assert ctx.L.svo_grid_route(ctx.h, case.blocked.ctypes.data, case.dist2.ctypes.data, C.byref(p), goals.ctypes.data, len(goals), None, 0,
                                C.byref(api.GridRouteOut(cost.ctypes.data)), None) == 0
    assert np.array_equal(cost, w.cost)
    # twice: the same bytes in every output
    first, second = {}, {}
    _eq(_run(ctx, case, keep=first), w, case.prm)
    _eq(_run(ctx, case, keep=second), w, case.prm)
    assert first == second and set(first) == set(_SENT)


@pytest.mark.gpu
def test_bad_calls_launch_nothing_and_leave_the_context_usable(ctx):
    import torch
    from stereo_vo_amd import api
    L = ctx.L
    case, w = random_want(63, 65, 0.25, True)
    good = case.prm
    n, ns, ng = good.na * good.nb, len(case.starts), len(case.goals)
    d = _Dev(case)
    O = api.GridRouteOut
    P = {k: b.data_ptr() + b.element_size() for k, b in d.bufs.items()}
    full = lambda **kw: O(**{**P, **kw})
    A = dict(blocked=d.blocked.data_ptr() + 1, dist2=d.dist2.data_ptr() + 4, goals=d.goals.data_ptr() + 4, n_goals=ng,
             starts=d.starts.data_ptr() + 4, n_starts=ns, ws=d.ws.data_ptr() + 8, counts=d.cnt.data_ptr() + 8)

    def dev(prm=good, out=None, null_prm=False, null_out=False, **kw):
        a = {**A, **kw}
        o = out if out is not None else full()
        p = _api_params(prm)
        return L.svo_grid_route_dev(ctx.h, a["blocked"], a["dist2"], None if null_prm else C.byref(p), a["goals"], a["n_goals"], a["starts"],
                                    a["n_starts"], a["ws"], None if null_out else C.byref(o), a["counts"])

    r = good._replace
    hcost = np.full((good.na, good.nb), 0x5555AAAA, np.uint32)
    hgoals = np.asarray(case.goals, np.uint32)

    def host(prm=good, blocked=case.blocked.ctypes.data, goals=hgoals.ctypes.data, out=None, null_out=False):
        o = out if out is not None else O(hcost.ctypes.data)
        return L.svo_grid_route(ctx.h, blocked, None, C.byref(_api_params(prm)), goals, ng, None, 0, None if null_out else C.byref(o), None)

    calls = [(lambda: dev(blocked=None), "null blocked"), (lambda: dev(null_prm=True), "null params"), (lambda: dev(goals=None), "null goals"),
             (lambda: dev(ws=None), "null workspace"), (lambda: dev(null_out=True), "null out"), (lambda: dev(out=full(cost=None)), "null cost"),
             (lambda: dev(starts=None), "null starts"),
             (lambda: dev(out=full(path=None)), "go together"), (lambda: dev(out=full(path_len=None)), "go together"),
             (lambda: dev(out=full(path_status=None)), "go together"), (lambda: dev(out=full(path=None, path_len=None)), "go together"),
             (lambda: dev(n_starts=0, starts=None), "n_starts == 0"),
             (lambda: dev(r(na=0)), "na outside"), (lambda: dev(r(na=8193)), "na outside"), (lambda: dev(r(nb=0)), "nb outside"),
             (lambda: dev(r(nb=8193)), "nb outside"), (lambda: dev(r(na=8192, nb=2049)), "na * nb"),
             (lambda: dev(r(near_r2=(1 << 26) + 1, near_weight=0)), "near_r2"), (lambda: dev(r(near_r2=1 << 10, near_weight=(1 << 10) + 1)), "near_weight * near_r2"),
             (lambda: dev(r(near_r2=3, near_weight=0xFFFFFFFF)), "near_weight * near_r2"),
             (lambda: dev(r(max_cost=0)), "max_cost"), (lambda: dev(r(max_cost=0x7F000001)), "max_cost"), (lambda: dev(r(max_cost=0xFFFFFFFF)), "max_cost"),
             (lambda: dev(r(max_rounds=0)), "max_rounds"), (lambda: dev(r(max_rounds=4097)), "max_rounds"),
             (lambda: dev(r(max_path=0)), "max_path"), (lambda: dev(r(max_path=(1 << 20) + 1)), "max_path"),
             (lambda: dev(r(resume=2)), "resume"), (lambda: dev(r(resume=-1)), "resume"),
             (lambda: dev(n_goals=0), "n_goals"), (lambda: dev(n_goals=65537), "n_goals"), (lambda: dev(n_starts=-1), "n_starts"),
             (lambda: dev(n_starts=4097), "n_starts"),
             (lambda: dev(out=full(cost=P["cost"] + 2)), "cost must be 4-byte"), (lambda: dev(dist2=A["dist2"] + 1), "dist2 must be 4-byte"),
             (lambda: dev(goals=A["goals"] + 2), "goals must be 4-byte"), (lambda: dev(starts=A["starts"] + 3), "starts must be 4-byte"),
             (lambda: dev(out=full(path=P["path"] + 2)), "path must be 4-byte"), (lambda: dev(out=full(path_len=P["path_len"] + 1)), "path_len must be 4-byte"),
             (lambda: dev(ws=A["ws"] + 4), "workspace must be 8-byte"), (lambda: dev(counts=A["counts"] + 4), "counts must be 8-byte"),
             (lambda: host(blocked=None), "null blocked"), (lambda: host(r(max_rounds=0)), "max_rounds"), (lambda: host(r(resume=1)), "resume"),
             (lambda: host(goals=None), "null goals"), (lambda: host(null_out=True), "null out"), (lambda: host(out=O(None)), "null cost"),
             (lambda: host(out=O(hcost.ctypes.data, None, hcost.ctypes.data, hcost.ctypes.data, hcost.ctypes.data)), "n_starts == 0")]
    ctx.profile_select("grid_route")
    for call, word in calls:
        assert call() == -1 and word in L.svo_last_error(ctx.h).decode(), (word, L.svo_last_error(ctx.h).decode())
    assert ctx.profile_read()[1] == 0
    ctx.sync()
    for k, (t, v) in _SENT.items():
        assert (d.bufs[k].cpu().numpy() == v).all(), k
    assert (d.ws.cpu().numpy() == 0x7F7F7F7F7F7F7F7F).all() and (d.cnt.cpu().numpy() == -1).all() and (hcost == 0x5555AAAA).all()
    # max_path is not looked at without starts; the boundaries' accepted sides in one call
    assert dev(r(max_path=0, near_r2=1 << 26, near_weight=0, max_cost=1, max_rounds=1), n_starts=0, starts=None,
               out=full(path=None, path_len=None, path_status=None)) == 0
    assert ctx.profile_read()[1] == 1
    ctx.profile_select(None)
    with pytest.raises(api.SvoError):
        ctx.grid_route(A["blocked"], _api_params(good), A["goals"], ng, cost_ptr=P["cost"])  # no workspace
    with pytest.raises(api.SvoError):
        ctx.grid_route_host(case.blocked, case.goals, max_rounds=0)
    with pytest.raises(ValueError):
        ctx.grid_route_host(case.blocked, case.goals, params=_api_params(good._replace(na=5)))
    # the context is what it was, and gives the route
    _eq(_run(ctx, case), w, case.prm)
    _eq(_run(ctx, case, "host"), w, case.prm)
