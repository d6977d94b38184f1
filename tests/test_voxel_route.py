"""The voxel map route (include/svo.h, "Voxel map route") against its restatement tests/voxel_route_ref.py, with == on
cost, next, path up to the written length, path_len, path_status and the counts; rounds_run is only bounded.

CPU: the restatement's two routes (Dijkstra, whole-array Bellman-Ford) agree on every case used below; open unweighted volumes follow
the closed form 80 a + 32 b + 32 c; a one-layer volume has the ground plan route's field; the constructed volumes are what they were
built to be; each deliberate misreading of the contract changes a result; the serpentine is as far from its goal as the GPU test
needs for both tile shapes; the pure entries and the refusals that need no context; stereo_vo_amd/host/voxel_route.h walked by
tests/sanitize/voxel_route_args_test.cpp under ASan + UBSan.
GPU: seeded volumes of seventeen shapes at three densities with and without dist2; the constructed volumes through both entries; one
round that cannot converge and the resumed calls that do; the one-layer volume against svo_grid_route_dev bit for bit; closed and
dist2 straight from the distance field's call; every optional output left out; a repeated call; bad calls.  Every device call runs
into a dirty workspace and sentinel-filled outputs whose guard elements stay, with closed, dist2, goals and starts between guard
elements.

ROUNDS.  route_np's sweep s gives every cell its final cost whose cheapest route of fewest moves has s moves; a round does at least
what a sweep does for every cell the round before changed something next to (the tile that lowered a cell wakes every tile that
sees it, itself included when its sweep bound cut it short), and one more round finds nothing to do; so max_rounds = sweeps + 2
always converges.  The random and constructed cases run with that bound, taken from the restatement.

Misreadings, cells that change on the restatement (volume "mixed": 64 x 17 x 9, density 0.25, dist2 0 .. 40 with a fifth 0xFFFF,
near_r2 16, near_weight 3, one goal of three on a closed cell, max_cost 2,068, the cost of the cell at the upper quartile; 5,552
cells reached, 45 of them at exactly max_cost): edge moves cutting corners 5,872 cost; vertex moves checking the three face cells only
3,075 cost; the penalty of the cell left 5,761 cost; weights 5-7-7 3,908 cost and 3-4-5 7,384 cost; 6 neighbours 5,506 cost and 18
neighbours 610 cost; the tie to the largest k 1,378 next; < max_cost 45 cost; a goal on a closed cell used 1 cost; 0xFFFF read as near
5,050 cost; j1 and j2 swapped in the goals' cell numbers 5,900 cost; axis 0 running on into the next row 578 cost.
"""
import ctypes as C
import functools
import time

import numpy as np
import pytest

import grid_route_ref as G
import voxel_route_ref as V
from test_host_sanitizers import _run_sanitized

MISREADINGS = {"corner_cut": ("cost", 5872), "vertex_faces": ("cost", 3075), "pen_left": ("cost", 5761), "w577": ("cost", 3908), "w345": ("cost", 7384),
               "six": ("cost", 5506), "eighteen": ("cost", 610), "tie_largest": ("next", 1378), "lt_max": ("cost", 45), "goal_closed": ("cost", 1),
               "none_near": ("cost", 5050), "swap12": ("cost", 5900), "row_wrap": ("cost", 578)}
OUTPUTS = ("next", "path")
VS = 0.25


def _freeze(r):
    for a in r[:5]:
        a.setflags(write=False)
    return r


def _bounded(case):
    """(the case with max_rounds set to the bound of the docstring, its restatement)"""
    w = V.route_np(case.closed, case.dist2, case.prm, case.goals, case.starts)
    rounds = w.sweeps + 2
    assert rounds <= 4096, rounds
    return case._replace(prm=case.prm._replace(max_rounds=rounds)), _freeze(w)


@functools.lru_cache(maxsize=None)
def random_want(dims, density, with_dist2):
    return _bounded(V.random_case(dims, density, with_dist2))


@functools.lru_cache(maxsize=None)
def constructed_want():
    return {name: _bounded(case) + (facts,) for name, (case, facts) in V.constructed().items()}


@functools.lru_cache(maxsize=None)
def serpentine_want():
    case = V.serpentine_case()
    return case, _freeze(V.route_np(*case))


RANDOM = [(dims, density, d2) for dims in V.SIZES for density in V.DENSITIES for d2 in (False, True)]


# ===================================================================================================== CPU
def test_the_two_routes_of_the_restatement_agree_on_every_case():
    reached = unreached = truncated = 0
    slowest = 0.0
    for dims, density, d2 in RANDOM:
        case, a = random_want(dims, density, d2)
        t0 = time.perf_counter()
        b = V.route_py(case.closed, case.dist2, case.prm, case.goals, case.starts)
        slowest = max(slowest, time.perf_counter() - t0)
        assert V.same(a, b), (dims, density, d2)
        assert sum(a.counts[1:4]) == dims[0] * dims[1] * dims[2] and a.counts[3] == int(case.closed.sum()) and a.counts[0] >= 1
        reached += a.counts[1]
        unreached += a.counts[2]
        truncated += int((a.path_status == V.TRUNCATED).sum())
    print("the heap Dijkstra's slowest volume: %.1f s" % slowest)
    # the cases are what the kernels' paths need: reached and cut-off cells, paths longer than max_path, several tiles and rounds
    assert reached > 500000 and unreached > 1000 and truncated >= 20
    assert random_want((128, 33, 17), 0.4, True)[0].prm.max_rounds > 64
    for name, (case, a, _) in constructed_want().items():
        assert V.same(a, V.route_py(case.closed, case.dist2, case.prm, case.goals, case.starts)), name
    case = V.misreading_case()
    assert V.same(V.route_np(*case), V.route_py(*case))
    case, w = serpentine_want()
    assert V.same(w, V.route_py(*case))


def test_open_unweighted_volumes_follow_the_closed_form():
    """With no closed cell and no penalty a route over coordinate differences a >= b >= c takes c vertex moves (9 * 16 = 144 each,
    against 112 + 80 for the edge and the face move it replaces and 240 for three face moves), b - c edge moves (7 * 16 = 112, against
    160 for two face moves) and a - b face moves (5 * 16 = 80): no route has fewer than a moves, every move changes at most one unit
    per axis, and replacing a move by one that changes more axes is always cheaper than adding a move, so the greedy count is the
    cheapest.  144 c + 112 (b - c) + 80 (a - b) = 80 a + 32 b + 32 c: the 5-7-9 chamfer distance times 16."""
    for dims, goal in (((64, 1, 1), (5, 0, 0)), ((64, 7, 5), (11, 3, 4)), ((64, 9, 9), (63, 0, 8)), ((128, 5, 12), (0, 0, 0))):
        c = np.zeros((dims[2], dims[1], dims[0]), bool)
        got = V.route_np(c, None, V.params(), [V.cell(c, *goal)])
        diff = np.stack(np.broadcast_arrays(np.abs(np.arange(dims[0]) - goal[0])[None, None, :], np.abs(np.arange(dims[1]) - goal[1])[None, :, None],
                                            np.abs(np.arange(dims[2]) - goal[2])[:, None, None]))
        s = np.sort(diff, axis=0)
        assert np.array_equal(got.cost, 80 * s[2] + 32 * s[1] + 32 * s[0]), dims
    assert V.open_cost(3, 5, 2) == 5 * 80 + 3 * 32 + 2 * 32 == 2 * 144 + 1 * 112 + 2 * 80


def _layer_case(d0, d1, density, with_dist2):
    """A one-layer volume and the ground plan grid it is under ia = j1, ib = j0 (cell numbers are the same)."""
    case = V.random_case((d0, d1, 1), density, with_dist2, seed=11)
    blocked = case.closed[0].astype(np.uint8)
    d2 = None if case.dist2 is None else np.where(case.dist2[0] == V.NONE16, G.NONE, case.dist2[0]).astype(np.uint32)
    gp = G.Params(d1, d0, case.prm.near_r2, case.prm.near_weight, case.prm.max_cost, case.prm.max_rounds, case.prm.max_path, 0)
    return case, G.Case(blocked, d2, gp, case.goals, case.starts)


def test_a_one_layer_volume_has_the_ground_plan_routes_field():
    """d2 = 1 leaves the eight moves of the layer, k = 9 + 3 (dj1 + 1) + (dj0 + 1), with weights 5 and 7 and the same two cells between
    the ends of a diagonal: the ground plan route with ia = j1, ib = j0, whose raster order of (dia, dib) is the order of these k."""
    code = np.full(256, 255, np.uint8)
    for k2, (dia, dib) in enumerate(G.MOVES):
        code[k2] = 9 + 3 * (dia + 1) + (dib + 1)
    code[8] = V.SELF
    for d0, d1 in ((64, 33), (128, 17)):
        for density in V.DENSITIES:
            for with_d2 in (False, True):
                case, g = _layer_case(d0, d1, density, with_d2)
                a, b = V.route_np(*case), G.route_np(*g)
                assert np.array_equal(a.cost[0], b.cost) and np.array_equal(a.next[0], code[b.next]), (d0, d1, density, with_d2)
                assert np.array_equal(a.path, b.path) and np.array_equal(a.path_len, b.path_len) and a.counts == b.counts


def test_the_constructed_volumes_are_what_they_were_built_to_be():
    for name, (case, a, facts) in constructed_want().items():
        if "counts" in facts:
            assert a.counts == facts["counts"], (name, a.counts)
        for (j0, j1, j2), value in facts.get("cost", {}).items():
            assert int(a.cost[j2, j1, j0]) == value, (name, (j0, j1, j2), int(a.cost[j2, j1, j0]))
        for (j0, j1, j2), k in facts.get("next", {}).items():
            assert int(a.next[j2, j1, j0]) == k, (name, (j0, j1, j2), int(a.next[j2, j1, j0]))
        assert list(a.path_status) == facts["status"], (name, list(a.path_status))
    cw = constructed_want()
    case, a, _ = cw["slab_hole"]
    assert V.cell(case.closed, 5, 7, 4) in a.path[0, :a.path_len[0]] and a.path[0, a.path_len[0] - 1] == 0
    case, a, _ = cw["penalty_corridor"]
    assert not set(a.path[0, :a.path_len[0]].tolist()) & {V.cell(case.closed, j0, 2, 0) for j0 in range(2, 7)} and a.path_len[0] == 9
    case, a, _ = cw["starts_and_max_path_1"]
    assert list(a.path_len[:4]) == [0, 0, 0, 1] and a.path_len[4] > 1
    case, a, _ = cw["no_wrap"]
    assert a.path_len[0] == 64


def test_every_misreading_of_the_contract_changes_a_result():
    case = V.misreading_case()
    assert V.dims_of(case.closed) == (64, 17, 9)
    right = V.route_np(*case)
    print("mixed: max_cost", case.prm.max_cost, "counts", right.counts)
    assert (right.cost == case.prm.max_cost).sum() >= 1 and right.counts[0] == 2 and right.counts[2] > 500
    got = {}
    for variant, (field, _) in MISREADINGS.items():
        wrong = V.route_np(*case, variant=variant)
        got[variant] = (field, int((getattr(right, field) != getattr(wrong, field)).sum()))
        assert got[variant][1] > 0, variant
    assert got == MISREADINGS, got
    assert set(MISREADINGS) == set(V.VARIANTS)


def test_the_serpentine_is_longer_than_three_tiles_for_both_tile_shapes():
    case, w = serpentine_want()
    d0, d1, d2 = V.dims_of(case.closed)
    assert w.counts == (1, 9 * 128 * 8 + 8 * 8, 0, 8 * (128 * 8 - 8), 1)
    assert list(w.path_status) == [V.OK, V.OK, V.OK] and w.path_len[2] == 1 and w.path_len[0] > 8 * 120
    for t in V.TILES:
        # round 1 runs the goal's tile and the 26 around it; what they can lower lies in tiles 0 and 1 along axis 0, so a cell three
        # or more tiles along has no cost after one round, and the volume has such cells
        assert d0 // t[0] > 3 and (w.cost[0, :, 3 * t[0]:] != V.NONE).all()


def _api_params(prm):
    from stereo_vo_amd import api
    return api.VoxelRouteParams(*prm)


def test_pure_entries_and_refusals_without_a_context():
    from stereo_vo_amd import api
    L = api.lib()
    d = api.voxel_route_default_params(0.1)
    assert (d.near_r2, d.near_weight, d.max_cost, d.max_rounds, d.max_path, d.resume) == (0, 0, 0x7F000000, 32, 4096, 0)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(api.SvoError):
            api.voxel_route_default_params(bad)
    assert L.svo_voxel_route_default_params(C.c_float(0.1), None) == -1
    ws = api.voxel_route_workspace_bytes
    # a header, two words per tile (whichever of the two tile shapes) and a byte per cell
    for dims in ((64, 1, 1), (128, 33, 17), (512, 128, 512), (2048, 2048, 256)):
        tiles = [-(-dims[0] // t[0]) * -(-dims[1] // t[1]) * -(-dims[2] // t[2]) for t in V.TILES]
        n = dims[0] * dims[1] * dims[2]
        assert ws(dims) % 8 == 0 and 64 + 8 * min(tiles) + n <= ws(dims) <= 64 + 8 * max(tiles) + n + 7, dims
    for dims in ((0, 1, 1), (65, 1, 1), (64, 2049, 1), (2048, 2048, 257), (64, 1, 0)):
        with pytest.raises(api.SvoError):
            ws(dims)
    n = C.c_size_t(5)
    assert L.svo_voxel_route_workspace_bytes(None, C.byref(n)) == -1 and n.value == 0
    assert (api.VOXEL_ROUTE_NONE, api.VOXEL_ROUTE_MAX_COST, api.VOXEL_ROUTE_NOT_CONVERGED, api.VOXEL_ROUTE_OUT_OF_VOLUME, api.VOXEL_ROUTE_SELF) == \
        (0xFFFFFFFF, 0x7F000000, 4, 3, 13)
    # cell_of: the distance query's rule 9, q = x / voxel_size in doubles from the widened f32, j = floor(q) - origin
    origin, dims = (-61, -3, -7), (128, 9, 13)
    f32 = np.float32
    for xyz in ((0.0, 0.0, 0.0), (-15.25, -0.75, -1.75), (16.74, 1.49, 1.49), (0.1, 0.2, 0.3), (-0.0001, 0.0, 0.0)):
        j = [int(np.floor(float(f32(x)) / float(f32(VS)))) - o for x, o in zip(xyz, origin)]
        assert all(0 <= a < b for a, b in zip(j, dims)), xyz
        assert api.voxel_occupancy_cell_of(VS, origin, dims, xyz) == j[0] + dims[0] * (j[1] + dims[1] * j[2]), xyz
    for xyz in ((-15.26, 0.0, 0.0), (16.75, 0.0, 0.0), (0.0, 1.5, 0.0), (0.0, 0.0, -1.76), (float("nan"), 0.0, 0.0), (float("inf"), 0.0, 0.0), (0.0, 3.0e5, 0.0)):
        with pytest.raises(api.SvoError):
            api.voxel_occupancy_cell_of(VS, origin, dims, xyz)
    for vs, o, dm in ((0.0, origin, dims), (VS, (1 << 20, 0, 0), dims), (VS, origin, (100, 9, 13))):
        with pytest.raises(api.SvoError):
            api.voxel_occupancy_cell_of(vs, o, dm, (0.0, 0.0, 0.0))
    # a null map is refused by both entries before anything else is looked at
    buf = (C.c_double * 12)()
    out = api.VoxelRouteOut(C.addressof(buf))
    d3 = np.array([64, 1, 1], np.int32)
    assert L.svo_voxel_occupancy_route_dev(None, buf, d3.ctypes.data, None, C.byref(d), buf, 1, None, 0, buf, C.byref(out), None) == -1
    assert L.svo_voxel_occupancy_route(None, buf, d3.ctypes.data, None, C.byref(d), buf, 1, None, 0, C.byref(out), None) == -1
    assert L.svo_voxel_occupancy_route_dev(None, None, None, None, None, None, 0, None, 0, None, None, None) == -1


def test_voxel_route_args_every_refusal_the_sizes_the_geometry_the_defaults_and_the_cell_statements(tmp_path):
    """host/voxel_route.h on the CPU under ASan + UBSan: every refusal at its boundary with code and exact message, the order of the
    refusals, the workspace size and layout, the tile counts and launch geometry at 64 x 1 x 1, at t - 1, t, t + 1 of each tile edge,
    at 2048 x 2048 x 256 and in size_t past 2^32, the defaults, cell_of against rule 9, and the header's per-cell statements relaxing
    a small volume to its fixed point against a brute-force Bellman-Ford written in the program."""
    _run_sanitized(tmp_path, "voxel_route_args_test", "voxel route args ok")


# ===================================================================================================== GPU
_SENT = {"cost": (np.int32, 0x5555AAAA), "next": (np.uint8, 0xBB), "path": (np.int32, 0x3333CCCC), "path_len": (np.int32, 0x77777777),
         "path_status": (np.uint8, 0xEE)}
_GROUP = {"next": ("next",), "path": ("path", "path_len", "path_status")}


class _Dev:
    """A case's device buffers: closed, dist2, goals and starts between guard elements (a guard read as a cell would be passable, and
    near), a dirty workspace and sentinel-filled outputs with a guard element before and behind each.  skip: of OUTPUTS, the outputs
    passed as NULL."""

    def __init__(self, case, skip=(), counts=True):
        import torch
        from stereo_vo_amd import api
        self.case, self.prm, self.skip, self.counts = case, case.prm, tuple(skip), counts
        self.dims = V.dims_of(case.closed)
        n, ns = case.closed.size, len(case.starts)
        self.n, self.ns = n, ns

        def guarded(a, t, guard):
            d = torch.full((len(a) + 2,), guard, dtype=t, device="cuda")
            if len(a):
                d[1:-1] = torch.from_numpy(np.ascontiguousarray(a)).cuda()
            return d

        self.words = V.pack(case.closed)
        self.closed = guarded(self.words.view(np.int64), torch.int64, 0)
        self.dist2 = None if case.dist2 is None else guarded(case.dist2.ravel().view(np.int16), torch.int16, 0)
        self.goals = guarded(np.asarray(case.goals, np.uint32).view(np.int32), torch.int32, 0)
        self.starts = guarded(np.asarray(case.starts, np.uint32).view(np.int32), torch.int32, 0)
        words = api.voxel_route_workspace_bytes(self.dims) // 8
        self.ws = torch.full((words + 2,), 0x7F7F7F7F7F7F7F7F, dtype=torch.int64, device="cuda")
        sizes = {"cost": n, "next": n, "path": ns * self.prm.max_path, "path_len": ns, "path_status": ns}
        self.bufs = {k: torch.full((sizes[k] + 2,), v, dtype=getattr(torch, np.dtype(t).name), device="cuda") for k, (t, v) in _SENT.items()}
        self.cnt = torch.full((10,), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()

    def call(self, vm, **over):
        p = _api_params(self.prm._replace(**over))
        ptr = {k: b.data_ptr() + b.element_size() for k, b in self.bufs.items()}
        for group in self.skip:
            for k in _GROUP[group]:
                ptr[k] = None
        if not self.ns:
            ptr["path"] = ptr["path_len"] = ptr["path_status"] = None
        vm.route(self.closed.data_ptr() + 8, self.dims, self.goals.data_ptr() + 4, len(self.case.goals), params=p,
                 dist2_ptr=None if self.dist2 is None else self.dist2.data_ptr() + 2, starts_ptr=self.starts.data_ptr() + 4 if self.ns else None,
                 n_starts=self.ns, workspace_ptr=self.ws.data_ptr() + 8, counts_ptr=self.cnt.data_ptr() + 8 if self.counts else None,
                 **{k + "_ptr": v for k, v in ptr.items()})
        vm.ctx.sync()

    def read(self, keep=None):
        """A V.Route with None for what was skipped; path rows keep their sentinel where nothing was written."""
        case, prm = self.case, self.prm
        w = self.ws.cpu().numpy()
        assert w[0] == w[-1] == 0x7F7F7F7F7F7F7F7F
        a = self.closed.cpu().numpy()
        assert a[0] == a[-1] == 0 and np.array_equal(a[1:-1].view(np.uint64), self.words)  # only read
        if self.dist2 is not None:
            assert np.array_equal(self.dist2.cpu().numpy()[1:-1].view(np.uint16).reshape(case.dist2.shape), case.dist2)
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
        shape = case.closed.shape
        return V.Route(u32(got["cost"]).reshape(shape), None if got["next"] is None else got["next"].reshape(shape),
                       None if got["path"] is None else u32(got["path"]).reshape(self.ns, prm.max_path), u32(got["path_len"]), got["path_status"],
                       tuple(int(v) for v in c[1:7]) if self.counts else None, None)


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


def _run(vm, case, how="dev", skip=(), counts=True, keep=None):
    if how == "host":
        d = _Dev(case)
        r = vm.route_host(d.closed.data_ptr() + 8, d.dims, case.goals, starts=case.starts if len(case.starts) else None,
                          dist2_ptr=None if d.dist2 is None else d.dist2.data_ptr() + 2, params=_api_params(case.prm))
        c = r["counts"]
        path = r.get("path")
        if path is not None:  # the host wrapper fills with NONE what the device tests fill with their sentinel
            written = np.arange(path.shape[1])[None, :] < np.minimum(r["path_len"], path.shape[1])[:, None]
            path = np.where(written, path, 0x3333CCCC).astype(np.uint32)
        return V.Route(r["cost"], r["next"], path, r.get("path_len"), r.get("path_status"),
                       tuple(c[k] for k in ("n_goals_used", "n_reached", "n_unreached", "n_closed", "converged", "rounds_run")), None)
    d = _Dev(case, skip, counts)
    d.call(vm)
    return d.read(keep)


@pytest.fixture
def vm(ctx):
    import stereo_vo_amd as S
    m = S.VoxelMap(ctx, voxel_size=VS, capacity_log2=8, max_depth=0.0)
    yield m
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dims", V.SIZES)
def test_random_volumes(vm, dims):
    for density in V.DENSITIES:
        for d2 in (False, True):
            case, w = random_want(dims, density, d2)
            got = _run(vm, case)
            print(dims, density, d2, "max_rounds", case.prm.max_rounds, "counts", got.counts)
            _eq(got, w, case.prm, (density, d2))


@pytest.mark.gpu
def test_constructed_volumes_through_both_entries(vm):
    for name, (case, w, facts) in constructed_want().items():
        if "counts" in facts:
            assert w.counts == facts["counts"], name
        for how in ("dev", "host"):
            got = _run(vm, case, how)
            print(name, how, got.counts)
            _eq(got, w, case.prm, (name, how))


@pytest.mark.gpu
def test_one_round_cannot_converge_and_resumed_calls_do(vm):
    case, w = serpentine_want()
    d0, d1, d2 = V.dims_of(case.closed)
    d = _Dev(case)
    d.call(vm)
    got = d.read()
    assert got.counts[:5] == (1, 0, 0, 0, 0) and got.counts[5] == 1, got.counts
    assert (got.next == 0xBB).all() and (got.path == 0x3333CCCC).all()  # not written
    assert (got.path_len == 0).all() and (got.path_status == V.NOT_CONVERGED).all()
    far = 3 * max(t[0] for t in V.TILES)
    assert (got.cost[:, :, far:] == V.NONE).all()
    some = got.cost != V.NONE
    assert some.sum() >= 8 * 8 and (got.cost[some] >= w.cost[some]).all() and got.cost[0, 0, 0] == 0
    # Every round carries the field at least through one more tile of the way (a tile's stretch of it is far shorter than the sweep
    # bound): the way crosses each of the nine open layers once, at most d0 / 8 + 2 tiles of either shape each, the holes included.
    per_call = 4
    bound = -(-(9 * (d0 // min(t[0] for t in V.TILES) + 2) + 2) // per_call)
    calls = 0
    while got.counts[4] == 0 and calls < bound:
        d.call(vm, resume=1, max_rounds=per_call)
        got = d.read()
        calls += 1
        some = got.cost != V.NONE
        assert (got.cost[some] >= w.cost[some]).all()
    print("resumed calls", calls, "of at most", bound)
    assert got.counts[4] == 1 and 2 <= calls
    _eq(got, w, case.prm._replace(max_rounds=per_call), "resumed")
    # a further resumed call finds nothing to do and gives the same again
    d.call(vm, resume=1, max_rounds=3)
    got = d.read()
    assert got.counts[5] == 0
    _eq(got, w, case.prm._replace(max_rounds=3), "after convergence")


@pytest.mark.gpu
@pytest.mark.parametrize("d0,d1", [(64, 33), (128, 17)])
def test_a_one_layer_volume_equals_the_ground_plan_route_bit_for_bit(ctx, vm, d0, d1):
    import torch
    from stereo_vo_amd import api
    for density in V.DENSITIES:
        for with_d2 in (False, True):
            case, g = _layer_case(d0, d1, density, with_d2)
            rounds = V.route_np(*case).sweeps + 2
            got = _run(vm, case._replace(prm=case.prm._replace(max_rounds=rounds)))
            n = d0 * d1
            blocked = torch.from_numpy(g.blocked.ravel().copy()).cuda()
            dist2 = None if g.dist2 is None else torch.from_numpy(g.dist2.ravel().view(np.int32).copy()).cuda()
            goals = torch.from_numpy(np.asarray(g.goals, np.uint32).view(np.int32).copy()).cuda()
            ws = torch.zeros(api.grid_route_workspace_bytes(d1, d0) // 8, dtype=torch.int64, device="cuda")
            cost = torch.full((n,), -2, dtype=torch.int32, device="cuda")
            cnt = torch.zeros(8, dtype=torch.int64, device="cuda")
            ctx.grid_route(blocked.data_ptr(), api.GridRouteParams(*g.prm._replace(max_rounds=rounds)), goals.data_ptr(), len(g.goals), workspace_ptr=ws.data_ptr(),
                           cost_ptr=cost.data_ptr(), dist2_ptr=None if dist2 is None else dist2.data_ptr(), counts_ptr=cnt.data_ptr())
            ctx.sync()
            assert cnt[4].item() == 1
            assert np.array_equal(cost.cpu().numpy().view(np.uint32), got.cost.ravel()), (density, with_d2)
            assert got.counts[:4] == tuple(cnt[:4].tolist())


@pytest.mark.gpu
def test_closed_and_dist2_straight_from_the_distance_field(vm):
    import torch
    from stereo_vo_amd import api
    dims = (128, 17, 9)
    n = dims[0] * dims[1] * dims[2]
    rng = np.random.default_rng(41)
    occupied = rng.random((dims[2], dims[1], dims[0])) < 0.02
    occupied[:, :, :2] = False
    bits = torch.from_numpy(V.pack(occupied).view(np.int64).copy()).cuda()
    ws = torch.zeros(api.voxel_distance_workspace_bytes(dims, False) // 8, dtype=torch.int64, device="cuda")
    d2 = torch.zeros(n, dtype=torch.int16, device="cuda")
    infl = torch.zeros(n // 64, dtype=torch.int64, device="cuda")
    vm.distance(bits.data_ptr(), dims, workspace_ptr=ws.data_ptr(), dist2_ptr=d2.data_ptr(), inflated_ptr=infl.data_ptr(), max_dist=2, inflate_radius=1.5 * VS)
    vm.ctx.sync()
    closed = V.unpack(infl.cpu().numpy().view(np.uint64), dims)
    dist2 = d2.cpu().numpy().view(np.uint16).reshape(closed.shape)
    assert closed.sum() > occupied.sum() > 50 and (dist2 == V.NONE16).sum() > 0 and not closed.ravel()[0]
    free = np.flatnonzero(~closed.ravel())
    prm = V.params(9, 5, max_path=512)
    case = V.Case(closed, dist2, prm, np.array([0, free[-1]], np.uint32), free[:: len(free) // 16].astype(np.uint32))
    case, w = _bounded(case)
    assert w.counts[1] > 1000 and (w.path_status == V.OK).sum() >= 8
    # the device arrays themselves go in: nothing is copied or converted on the way
    r = vm.route_host(infl.data_ptr(), dims, case.goals, starts=case.starts, dist2_ptr=d2.data_ptr(), params=_api_params(case.prm))
    assert np.array_equal(r["cost"], w.cost) and np.array_equal(r["next"], w.next) and np.array_equal(r["path_len"], w.path_len)
    assert np.array_equal(r["path"], w.path) and tuple(r["counts"][k] for k in api.VOXEL_ROUTE_COUNTS[:5]) == w.counts
    _eq(_run(vm, case), w, case.prm, "guarded copies")
    # the occupancy bits themselves fit as closed
    bare = V.Case(occupied, None, V.params(), case.goals, np.zeros(0, np.uint32))
    bare, wb = _bounded(bare)
    r = vm.route_host(bits.data_ptr(), dims, bare.goals, params=_api_params(bare.prm))
    assert np.array_equal(r["cost"], wb.cost) and np.array_equal(r["next"], wb.next) and "path" not in r


@pytest.mark.gpu
def test_optional_outputs_a_repeated_call_and_the_profile_bracket(ctx, vm):
    case, w = random_want((64, 17, 9), 0.25, True)
    ctx.profile_select("voxel_route")
    for skip in [(k,) for k in OUTPUTS] + [OUTPUTS]:
        got = _run(vm, case, skip=skip)
        assert (got.next is None) == ("next" in skip) and (got.path is None) == ("path" in skip)
        _eq(got, w, case.prm, skip)
    assert ctx.profile_read()[1] == 3
    ctx.profile_select(None)
    _eq(_run(vm, case, counts=False), w, case.prm, "no counts")
    _eq(_run(vm, case, skip=OUTPUTS, counts=False), w, case.prm, "cost alone")
    nostarts = case._replace(starts=np.zeros(0, np.uint32))
    _eq(_run(vm, nostarts), w, case.prm, "no starts")
    _eq(_run(vm, case, "host"), w, case.prm, "host")
    # 4096 starts, every status
    rng = np.random.default_rng(5)
    many = case._replace(starts=rng.integers(0, case.closed.size + 40, 4096).astype(np.uint32), prm=case.prm._replace(max_path=12))
    ww = V.route_np(*many)
    assert {V.OK, V.TRUNCATED, V.UNREACHED, V.OUT_OF_VOLUME} == set(ww.path_status.tolist())
    _eq(_run(vm, many), ww, many.prm, "4096 starts")
    # twice: the same bytes in every output
    first, second = {}, {}
    _eq(_run(vm, case, keep=first), w, case.prm)
    _eq(_run(vm, case, keep=second), w, case.prm)
    assert first == second and set(first) == set(_SENT)


@pytest.mark.gpu
def test_bad_calls_launch_nothing_and_leave_the_context_usable(ctx, vm):
    from stereo_vo_amd import api
    L = ctx.L
    case, w = random_want((64, 17, 9), 0.25, True)
    good = case.prm
    ns, ng = len(case.starts), len(case.goals)
    d = _Dev(case)
    O = api.VoxelRouteOut
    P = {k: b.data_ptr() + b.element_size() for k, b in d.bufs.items()}
    full = lambda **kw: O(**{**P, **kw})
    A = dict(closed=d.closed.data_ptr() + 8, dims=d.dims, dist2=d.dist2.data_ptr() + 2, goals=d.goals.data_ptr() + 4, n_goals=ng,
             starts=d.starts.data_ptr() + 4, n_starts=ns, ws=d.ws.data_ptr() + 8, counts=d.cnt.data_ptr() + 8)

    def dev(prm=good, out=None, null_prm=False, null_out=False, **kw):
        a = {**A, **kw}
        o = out if out is not None else full()
        p = _api_params(prm)
        dm = None if a["dims"] is None else np.array(a["dims"], np.int32)
        return L.svo_voxel_occupancy_route_dev(vm.h, a["closed"], None if dm is None else dm.ctypes.data, a["dist2"], None if null_prm else C.byref(p),
                                               a["goals"], a["n_goals"], a["starts"], a["n_starts"], a["ws"], None if null_out else C.byref(o), a["counts"])

    r = good._replace
    hcost = np.full(case.closed.shape, 0x5555AAAA, np.uint32)
    hgoals = np.asarray(case.goals, np.uint32)
    dm = np.array(d.dims, np.int32)

    def host(prm=good, closed=A["closed"], goals=hgoals.ctypes.data, out=None, null_out=False):
        o = out if out is not None else O(hcost.ctypes.data)
        return L.svo_voxel_occupancy_route(vm.h, closed, dm.ctypes.data, None, C.byref(_api_params(prm)), goals, ng, None, 0, None if null_out else C.byref(o), None)

    calls = [(lambda: dev(null_prm=True), "null params"),
             (lambda: dev(r(near_r2=254 * 254 + 1, near_weight=0)), "near_r2"), (lambda: dev(r(near_r2=1 << 10, near_weight=(1 << 10) + 1)), "near_weight * near_r2"),
             (lambda: dev(r(near_r2=3, near_weight=0xFFFFFFFF)), "near_weight * near_r2"),
             (lambda: dev(r(max_cost=0)), "max_cost"), (lambda: dev(r(max_cost=0x7F000001)), "max_cost"), (lambda: dev(r(max_cost=0xFFFFFFFF)), "max_cost"),
             (lambda: dev(r(max_rounds=0)), "max_rounds"), (lambda: dev(r(max_rounds=4097)), "max_rounds"),
             (lambda: dev(r(max_path=0)), "max_path"), (lambda: dev(r(max_path=(1 << 20) + 1)), "max_path"),
             (lambda: dev(r(resume=2)), "resume"), (lambda: dev(r(resume=-1)), "resume"),
             (lambda: dev(dims=None), "null dims"), (lambda: dev(dims=(0, 17, 9)), "dims outside"), (lambda: dev(dims=(64, 2049, 9)), "dims outside"),
             (lambda: dev(dims=(65, 17, 9)), "multiple of 64"), (lambda: dev(dims=(2048, 2048, 257)), "beyond 2^30"),
             (lambda: dev(closed=None), "null closed"), (lambda: dev(closed=A["closed"] + 4), "closed must be 8-byte"),
             (lambda: dev(goals=None), "null goals"), (lambda: dev(n_goals=0), "n_goals"), (lambda: dev(n_goals=65537), "n_goals"),
             (lambda: dev(n_starts=-1), "n_starts"), (lambda: dev(n_starts=4097), "n_starts"), (lambda: dev(starts=None), "null starts"),
             (lambda: dev(n_starts=0, out=full(path=None, path_len=None, path_status=None)), "starts with n_starts == 0"),
             (lambda: dev(ws=None), "null workspace"), (lambda: dev(null_out=True), "null out"), (lambda: dev(out=full(cost=None)), "null cost"),
             (lambda: dev(out=full(path=None)), "go together"), (lambda: dev(out=full(path_len=None)), "go together"),
             (lambda: dev(out=full(path_status=None)), "go together"), (lambda: dev(out=full(path=None, path_len=None)), "go together"),
             (lambda: dev(n_starts=0, starts=None), "path outputs with n_starts == 0"),
             (lambda: dev(out=full(cost=P["cost"] + 2)), "cost must be 4-byte"), (lambda: dev(goals=A["goals"] + 2), "goals must be 4-byte"),
             (lambda: dev(starts=A["starts"] + 3), "starts must be 4-byte"), (lambda: dev(out=full(path=P["path"] + 2)), "path must be 4-byte"),
             (lambda: dev(out=full(path_len=P["path_len"] + 1)), "path_len must be 4-byte"), (lambda: dev(dist2=A["dist2"] + 1), "dist2 must be 2-byte"),
             (lambda: dev(ws=A["ws"] + 4), "workspace must be 8-byte"), (lambda: dev(counts=A["counts"] + 4), "counts must be 8-byte"),
             # the order: params before dims before closed before the lists before the workspace before out before the alignments
             (lambda: dev(r(max_rounds=0), dims=None, closed=None), "max_rounds"), (lambda: dev(dims=None, closed=None), "null dims"),
             (lambda: dev(closed=None, goals=None), "null closed"), (lambda: dev(goals=None, ws=None), "null goals"),
             (lambda: dev(ws=None, null_out=True), "null workspace"), (lambda: dev(out=full(cost=None, path=None)), "null cost"),
             (lambda: dev(out=full(path=None, cost=P["cost"] + 2)), "go together"), (lambda: dev(out=full(cost=P["cost"] + 2), counts=A["counts"] + 4), "cost must be"),
             (lambda: host(closed=None), "null closed"), (lambda: host(r(max_rounds=0)), "max_rounds"), (lambda: host(r(resume=1)), "resume needs"),
             (lambda: host(goals=None), "null goals"), (lambda: host(null_out=True), "null out"), (lambda: host(out=O(None)), "null cost"),
             (lambda: host(out=O(hcost.ctypes.data, None, hcost.ctypes.data, hcost.ctypes.data, hcost.ctypes.data)), "n_starts == 0")]
    ctx.profile_select("voxel_route")
    for call, word in calls:
        assert call() == -1 and word in L.svo_last_error(ctx.h).decode(), (word, L.svo_last_error(ctx.h).decode())
    assert ctx.profile_read()[1] == 0
    ctx.sync()
    for k, (t, v) in _SENT.items():
        assert (d.bufs[k].cpu().numpy() == v).all(), k
    assert (d.ws.cpu().numpy() == 0x7F7F7F7F7F7F7F7F).all() and (d.cnt.cpu().numpy() == -1).all() and (hcost == 0x5555AAAA).all()
    # max_path is not looked at without starts; the boundaries' accepted sides in one call
    assert dev(r(max_path=0, near_r2=254 * 254, near_weight=0, max_cost=1, max_rounds=1), n_starts=0, starts=None,
               out=full(path=None, path_len=None, path_status=None)) == 0
    assert ctx.profile_read()[1] == 1
    ctx.profile_select(None)
    with pytest.raises(api.SvoError):
        vm.route(A["closed"], d.dims, A["goals"], ng, params=_api_params(good), cost_ptr=P["cost"])  # no workspace
    with pytest.raises(api.SvoError):
        vm.route_host(A["closed"], d.dims, case.goals, max_rounds=0)
    with pytest.raises(api.SvoError):
        vm.route_host(A["closed"], d.dims, case.goals, resume=1)
    # the context is what it was, and gives the route
    _eq(_run(vm, case), w, case.prm)
    _eq(_run(vm, case, "host"), w, case.prm)
