"""The gap the ground plan surface closes, shown on a terrace in a voxel map (include/svo.h, "Ground plan surface").

The terrace of tests/grid_surface_ref.py (two plateaus a metre apart, a ramp of 0.1 per cell across the ledge) is inserted as a cloud,
one record per cell, into a map of 0.25-unit voxels; the ground plan is 12 x 24 cells of 0.5: the terrace and four columns nobody has
seen.  The vehicle stands on the upper plateau; the route's start is on the lower one.

CPU: the chained restatements alone (voxel_ref, voxel_grid_ref, grid_surface_ref, grid_clearance_ref, grid_route_ref) show the facts:
every cell along the ledge is LEVEL; without the surface the path crosses the ledge where there is no ramp; with it the path climbs
the ramp's lane; with the ramp removed the start is unreachable.
GPU: grid -> clearance -> route over the grid's cls, and grid -> surface -> clearance with SVO_GRID_SURFACE_SOURCES -> route ->
frontiers -> view over cls_out, each chain enqueued on the context's stream with nothing read back in between; every output of both
chains equals the chained restatements with ==, and the same facts hold on what the device gave.
"""
import functools

import numpy as np
import pytest

import grid_clearance_ref as C
import grid_frontier_ref as F
import grid_route_ref as R
import grid_surface_ref as S
import grid_view_ref as W
import voxel_grid_ref as VG
import voxel_ref as V

VS, LOG2 = 0.25, 12
T = S.TERRACE
NA, NB = T["na"], T["nb"] + 4
GRID = VG.Params(1, -1, 1.0, 0.0, 2, NA, NB, -1.0, 2.0, 0.3, 1)  # y down; a = z from 1.0, b = x from 0; cells of two voxels
IDENT = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float64)
START, VEHICLE = 1 * NB + 2, 1 * NB + 17  # on the lower and on the upper plateau, three rows from the ramp
MAX_PATH, ROUNDS, MAX_FRONTIERS, MAX_RANGE = 64, 64, 16, 6
SPRM = S.Params(NA, NB, 1 << 1, 0.5, T["max_step"], S.radius_for(2), S.INF, 0)
RPRM = R.Params(NA, NB, 0, 0, R.MAX_COST, ROUNDS, MAX_PATH, 0)
FPRM = F.Params(NA, NB, 1 << F.LEVEL, 1 << F.UNKNOWN, 2, MAX_FRONTIERS)  # FREE stays LEVEL: a STEP cell is no frontier
VPRM = W.Params(NA, NB, 1 << W.OBSTACLE, 1 << W.UNKNOWN, MAX_RANGE, 16, 1)  # OPAQUE stays OBSTACLE: a kerb does not block sight
OK, UNREACHED = 0, 2  # SVO_GRID_ROUTE_OK, SVO_GRID_ROUTE_UNREACHED


def cprm(source_mask):
    return C.Params(NA, NB, source_mask, 8, 0.5, 0.0)


@functools.lru_cache(maxsize=None)
def cloud(ramp):
    """One record per cell of the terrace, well inside the cell's first voxel, at the height -y = top."""
    top = S.terrace_tops(ramp)
    ia, ib = np.meshgrid(np.arange(T["na"]), np.arange(T["nb"]), indexing="ij")
    x, y, z = 0.5 * ib + 0.1, -top.astype(np.float64), 1.0 + 0.5 * ia + 0.1
    p = V.records(x.ravel().astype(np.float32), y.ravel().astype(np.float32), z.ravel().astype(np.float32), np.full(ia.size, 0x40 << 24, np.uint32))
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def restated(ramp, surface):
    """The chain on the restatements alone: a dict of what every step gives."""
    g = VG.grid_np(V.insert_np(cloud(ramp), IDENT, VS), GRID, VS)
    w = {"grid": g}
    cls = g.cls
    if surface:
        w["surface"] = S.surface_np(g.cls, g.top, SPRM)
        cls = w["surface"].cls_out
    w["clearance"] = C.clearance_np(cls, cprm(S.SOURCES if surface else 1 << 2))
    w["route"] = R.route_np(w["clearance"].blocked, None, RPRM, np.array([VEHICLE], np.uint32), np.array([START], np.uint32))
    if surface:
        w["frontiers"] = F.frontiers_np(cls, w["clearance"].blocked, w["route"].cost, FPRM)
        w["view"] = W.views_np(cls, w["frontiers"].goal_cells, w["route"].cost, VPRM)
    return w


def _path(route):
    return [divmod(int(c), NB) for c in route.path[0, :int(route.path_len[0])]]


def _facts(plain, refined, closed):
    """plain: the chain without the surface; refined: with it; closed: with it and the ramp removed.  Each a dict as restated() gives."""
    ledge, lane = T["ledge"], range(*T["lane_rows"])
    g = plain["grid"]
    assert (g.cls[:, :T["nb"]] == VG.LEVEL).all() and (g.cls[:, T["nb"]:] == VG.UNKNOWN).all()  # the ledge's cells are LEVEL, all of them
    assert (np.abs(g.top[:, :T["nb"]].astype(np.float64) - S.terrace_tops().astype(np.float64)) < 1e-5).all()
    assert abs(float(g.top[0, ledge]) - float(g.top[0, ledge - 1]) - 1.0) < 1e-5
    # without the surface nothing is in the way: the path runs straight along its row and over the ledge, a metre up in one move
    assert plain["clearance"].counts[0] == 0 and not plain["clearance"].blocked.any()
    p = _path(plain["route"])
    assert plain["route"].path_status[0] == OK and p == [(1, ib) for ib in range(2, 18)]
    assert (1, ledge - 1) in p and (1, ledge) in p and 1 not in range(*T["ramp_rows"])
    # with it the ledge and the ramp's sides are sources, the lane is not, and the path climbs the lane
    s = refined["surface"]
    assert np.array_equal(s.cls_out[:, :T["nb"]], S.surface_np(*S.constructed()["terrace"]).cls_out) and s.counts[1] == 24
    assert np.array_equal(refined["clearance"].blocked == 2, s.cls_out == S.STEP)
    p = _path(refined["route"])
    assert refined["route"].path_status[0] == OK and p[0] == divmod(START, NB) and p[-1] == divmod(VEHICLE, NB)
    assert all(s.cls_out[c] == 1 for c in p)
    assert refined["route"].cost[divmod(START, NB)] > plain["route"].cost[divmod(START, NB)] == 15 * 5 * 16  # the detour costs
    crossing = [c for c in p if ledge - 2 <= c[1] <= ledge]
    assert len(crossing) >= 3 and all(ia in lane for ia, _ in crossing)
    # no move climbs the ledge: an edge move rises at most max_step, a diagonal one passes between two cells that are each that near
    rise = [(abs(float(g.top[a]) - float(g.top[b])), a[0] != b[0] and a[1] != b[1]) for a, b in zip(p, p[1:])]
    assert all(d <= (2 if diagonal else 1) * T["max_step"] for d, diagonal in rise)
    # the frontier is the upper plateau's last column, and it is seen from
    assert refined["frontiers"].counts[5] >= 1 and refined["view"].counts[0] >= 1 and refined["view"].best[2] > 0
    assert all(c % NB == T["nb"] - 1 for c in refined["frontiers"].goal_cells if c != F.NONE)
    # with the ramp removed the ledge is closed from edge to edge, and the route says so
    s = closed["surface"]
    assert (s.cls_out[:, ledge - 1:ledge + 1] == S.STEP).all() and s.counts[1] == 2 * NA
    r = closed["route"]
    assert r.path_status[0] == UNREACHED and r.path_len[0] == 0 and r.cost[divmod(START, NB)] == R.NONE
    assert (r.cost[:, :ledge - 1] == R.NONE).all() and (r.cost[:, ledge + 1:] != R.NONE).all()


def test_the_restatements_show_the_gap_and_its_closing():
    _facts(restated(True, False), restated(True, True), restated(False, True))
    for ramp, surface in ((True, False), (True, True), (False, True)):
        w = restated(ramp, surface)
        assert VG.same(w["grid"], VG.grid_py(V.insert_np(cloud(ramp), IDENT, VS), GRID, VS))
        if surface:
            assert S.same(w["surface"], S.as_surface(S.surface_py(w["grid"].cls, w["grid"].top, SPRM), SPRM))


def _chain(ctx, ramp, surface):
    """The chain on the device, nothing read back before the last step is enqueued; returns what restated() returns."""
    import torch
    import stereo_vo_amd as SV
    from stereo_vo_amd import api
    from test_grid_clearance import _api_params as clearance_params
    from test_grid_frontier import _api_params as frontier_params
    from test_grid_route import _api_params as route_params
    from test_grid_surface import _api_params as surface_params
    from test_grid_view import _api_params as view_params
    n = NA * NB
    i32 = lambda count, fill: torch.full((count,), fill, dtype=torch.int32, device="cuda")
    u8 = lambda count, fill: torch.full((count,), fill, dtype=torch.uint8, device="cuda")
    i64 = lambda count, fill: torch.full((count,), fill, dtype=torch.int64, device="cuda")
    vm = SV.VoxelMap(ctx, voxel_size=VS, capacity_log2=LOG2, max_depth=0.0)
    pts = torch.from_numpy(np.ascontiguousarray(cloud(ramp)).view(np.int32).reshape(-1, 4).copy()).cuda()
    vm.insert(pts.data_ptr(), len(cloud(ramp)), m12=IDENT)
    gws, gcnt = i64(api.voxel_grid_workspace_bytes(NA, NB) // 8, 0x7F7F7F7F7F7F7F7F), i64(8, -1)
    cls, top, bottom, inten, nvox, npts = u8(n, 0xAA), i32(n, 0x5555AAAA), i32(n, 0x3333CCCC), u8(n, 0xBB), i32(n, 0x77777777), i64(n, 0x6666666666666666)
    cls_out, step, relief, support, scnt = u8(n, 0xBB), i32(n, 0x77777777), i32(n, 0x5555AAAA), torch.full((n,), 0x3333, dtype=torch.int16, device="cuda"), i64(8, -1)
    offsets, d2, near, clr, blk, ccnt = i32(n, 0x7F7F7F7F), i32(n, 0x5555AAAA), i32(n, 0x3333CCCC), i32(n, 0x77777777), u8(n, 0xBB), i64(8, -1)
    rws, cost, nxt = i64(api.grid_route_workspace_bytes(NA, NB) // 8, 0x7F7F7F7F7F7F7F7F), i32(n, 0x5555AAAA), u8(n, 0xBB)
    path, plen, status, rcnt = i32(MAX_PATH, 0x3333CCCC), i32(1, 0x77777777), u8(1, 0xEE), i64(8, -1)
    goals = torch.from_numpy(np.array([VEHICLE], np.uint32).view(np.int32)).cuda()
    starts = torch.from_numpy(np.array([START], np.uint32).view(np.int32)).cuda()
    fws = i64(api.grid_frontier_workspace_bytes(NA, NB, MAX_FRONTIERS) // 8, 0x7F7F7F7F7F7F7F7F)
    frec, goal_cells, label, fcnt = i64(6 * MAX_FRONTIERS, 0x5A5A5A5A5A5A5A5A), i32(MAX_FRONTIERS, 0x3333CCCC), i32(n, 0x5555AAAA), i64(8, -1)
    vws = i64(api.grid_view_workspace_bytes(NA, NB, MAX_FRONTIERS) // 8, 0x7F7F7F7F7F7F7F7F)
    vrec, order, best, seen, vcnt = i64(4 * MAX_FRONTIERS, 0x5A5A5A5A5A5A5A5A), i32(MAX_FRONTIERS, 0x3333CCCC), i32(4, 0x77771111), i32(n, 0x5555AAAA), i64(8, -1)
    torch.cuda.synchronize()
    # everything from here to the sync is enqueued on the context's stream, each step reading the last one's device outputs
    vm.grid(api.VoxelGridParams(*GRID), workspace_ptr=gws.data_ptr(), cls_ptr=cls.data_ptr(), top_ptr=top.data_ptr(), bottom_ptr=bottom.data_ptr(),
            intensity_ptr=inten.data_ptr(), n_voxels_ptr=nvox.data_ptr(), n_points_ptr=npts.data_ptr(), counts_ptr=gcnt.data_ptr())
    used = cls
    if surface:
        ctx.grid_surface(cls.data_ptr(), top.data_ptr(), surface_params(SPRM), cls_out_ptr=cls_out.data_ptr(), step_ptr=step.data_ptr(),
                         relief_ptr=relief.data_ptr(), support_ptr=support.data_ptr(), counts_ptr=scnt.data_ptr())
        used = cls_out
    ctx.grid_clearance(used.data_ptr(), clearance_params(cprm(api.GRID_SURFACE_SOURCES if surface else 1 << api.VOXEL_GRID_OBSTACLE)),
                       workspace_ptr=offsets.data_ptr(), dist2_ptr=d2.data_ptr(), nearest_ptr=near.data_ptr(), clearance_ptr=clr.data_ptr(),
                       blocked_ptr=blk.data_ptr(), counts_ptr=ccnt.data_ptr())
    ctx.grid_route(blk.data_ptr(), route_params(RPRM), goals.data_ptr(), 1, workspace_ptr=rws.data_ptr(), cost_ptr=cost.data_ptr(), next_ptr=nxt.data_ptr(),
                   starts_ptr=starts.data_ptr(), n_starts=1, path_ptr=path.data_ptr(), path_len_ptr=plen.data_ptr(), path_status_ptr=status.data_ptr(),
                   counts_ptr=rcnt.data_ptr())
    if surface:
        ctx.grid_frontiers(used.data_ptr(), frontier_params(FPRM), blocked_ptr=blk.data_ptr(), cost_ptr=cost.data_ptr(), workspace_ptr=fws.data_ptr(),
                           frontiers_ptr=frec.data_ptr(), goal_cells_ptr=goal_cells.data_ptr(), label_ptr=label.data_ptr(), counts_ptr=fcnt.data_ptr())
        ctx.grid_view(used.data_ptr(), goal_cells.data_ptr(), MAX_FRONTIERS, view_params(VPRM), cost_ptr=cost.data_ptr(), workspace_ptr=vws.data_ptr(),
                      records_ptr=vrec.data_ptr(), order_ptr=order.data_ptr(), best_ptr=best.data_ptr(), seen_ptr=seen.data_ptr(), counts_ptr=vcnt.data_ptr())
    ctx.sync()
    host = lambda t, kind=None, shape=(NA, NB): (t.cpu().numpy() if kind is None else t.cpu().numpy().view(kind)).reshape(shape)
    tally = lambda t, k: tuple(int(v) for v in t.cpu()[:k])
    got = {"grid": VG.Grid(host(cls), host(top, np.float32), host(bottom, np.float32), host(inten), host(nvox, np.uint32), host(npts, np.uint64), tally(gcnt, 5))}
    if surface:
        got["surface"] = S.Surface(host(cls_out), host(step, np.float32), host(relief, np.float32), host(support, np.uint16), tally(scnt, 6))
    got["clearance"] = C.Clearance(host(d2, np.uint32), host(near, np.uint32), host(clr, np.float32), host(blk), tally(ccnt, 4))
    got["route"] = R.Route(host(cost, np.uint32), host(nxt), host(path, np.uint32, (1, MAX_PATH)), host(plen, np.uint32, (1,)), host(status, None, (1,)),
                           tally(rcnt, 6))
    if surface:
        got["frontiers"] = {"frontiers": frec.cpu().numpy().view(F.RECORD), "goal_cells": host(goal_cells, np.uint32, (MAX_FRONTIERS,)),
                            "label": host(label, np.uint32), "counts": tally(fcnt, 8)}
        got["view"] = {"records": vrec.cpu().numpy().view(W.RECORD), "order": host(order, np.uint32, (MAX_FRONTIERS,)), "best": host(best, np.uint32, (4,)),
                       "seen": host(seen, np.uint32), "counts": tally(vcnt, 8)}
    vm.close()
    return got


def _equal(got, w):
    from test_grid_clearance import _eq as clearance_eq
    from test_grid_frontier import _eq as frontier_eq
    from test_grid_route import _eq as route_eq
    from test_grid_surface import _eq as surface_eq
    from test_grid_view import _eq as view_eq
    from test_voxel_grid import _eq as grid_eq
    assert set(got) == set(w)
    grid_eq(got["grid"], w["grid"])
    if "surface" in w:
        surface_eq(got["surface"], w["surface"])
    clearance_eq(got["clearance"], w["clearance"])
    route_eq(got["route"], w["route"], RPRM)
    if "frontiers" in w:
        frontier_eq(got["frontiers"], w["frontiers"])
        view_eq(got["view"], w["view"])


@pytest.mark.gpu
def test_the_route_crosses_the_ledge_without_the_surface_and_climbs_the_ramp_with_it(ctx):
    chains = {}
    for ramp, surface in ((True, False), (True, True), (False, True)):
        got, w = _chain(ctx, ramp, surface), restated(ramp, surface)
        print("ramp", ramp, "surface", surface, "route counts", got["route"].counts, "status", got["route"].path_status, "len", got["route"].path_len,
              "surface counts", got["surface"].counts if surface else None)
        _equal(got, w)
        chains[ramp, surface] = got
    # the same facts on what the device gave: its frontiers and its view as the Results the facts read
    for got in (chains[True, True], chains[False, True]):
        got["frontiers"] = F.Result(got["frontiers"]["frontiers"], got["frontiers"]["goal_cells"], got["frontiers"]["label"], got["frontiers"]["counts"])
        got["view"] = W.Result(got["view"]["records"], got["view"]["order"], got["view"]["best"], got["view"]["seen"], got["view"]["counts"])
    _facts(chains[True, False], chains[True, True], chains[False, True])
