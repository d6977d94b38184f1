"""The planning cycle down to something a vehicle can follow (include/svo.h, "Ground plan waypoints"): grid -> surface ->
clearance with an inflation -> route to a goal -> waypoints, each step enqueued on the context's stream and reading the last one's
DEVICE outputs, nothing read back in between.

The scene is a flat floor of 24 x 40 cells of 0.5 in a voxel map of 0.25-unit voxels, with a wall a metre high along column 20 but for
a gap of four cells; the start is on one side, the goal on the other.

CPU: the chained restatements alone show the scene: the wall is OBSTACLE from edge to edge but for the gap, the inflation leaves two
rows of the gap, the route passes it.
GPU: every step equals the chained restatements with ==; way_status is 0 and no step is forced; the waypoints are the restatement's, far
fewer than the path's cells; a host walk of every segment finds it CLEAR; a waypoint lies at the gap; length is at most the staircase's
Euclidean length; with min_dist2 and the clearance's dist2 the segments keep that distance wherever a segment spans more than one path
entry.
"""
import functools
import math

import numpy as np
import pytest

import grid_clearance_ref as C
import grid_route_ref as R
import grid_surface_ref as S
import grid_waypoints_ref as G
import voxel_grid_ref as VG
import voxel_ref as V

VS, LOG2 = 0.25, 13
NA, NB, WALL, GAP = 24, 40, 20, range(2, 6)
GRID = VG.Params(1, -1, 1.0, 0.0, 2, NA, NB, -1.0, 2.0, 0.3, 1)  # y down; a = z from 1.0, b = x from 0; cells of two voxels
IDENT = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float64)
START, GOAL = 20 * NB + 4, 20 * NB + 36  # the straight line between them meets the wall
MAX_PATH, ROUNDS, MAX_WAY, MAX_LOOK, MIN_DIST2 = 128, 64, 32, 64, 4
SPRM = S.Params(NA, NB, 1 << 1, 0.5, 0.35, S.radius_for(2), S.INF, 0)
CPRM = C.Params(NA, NB, S.SOURCES, 8, 0.5, 0.5)  # the inflation: one cell
RPRM = R.Params(NA, NB, 0, 0, R.MAX_COST, ROUNDS, MAX_PATH, 0)
WPRM = G.Params(NA, NB, MAX_PATH, MAX_LOOK, 0, MAX_WAY, 0.5)


@functools.lru_cache(maxsize=None)
def cloud():
    """One record per cell on the floor, well inside the cell's first voxel, and one a metre up on every cell of the wall."""
    ia, ib = np.meshgrid(np.arange(NA), np.arange(NB), indexing="ij")
    wall = (ib == WALL) & ~np.isin(ia, list(GAP))
    ia, ib = np.concatenate([ia.ravel(), ia[wall]]), np.concatenate([ib.ravel(), ib[wall]])
    up = np.concatenate([np.zeros(NA * NB), np.ones(int(wall.sum()))])
    x, y, z = 0.5 * ib + 0.1, -up - 0.01, 1.0 + 0.5 * ia + 0.1
    p = V.records(x.astype(np.float32), y.astype(np.float32), z.astype(np.float32), np.full(len(x), 0x40 << 24, np.uint32))
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def restated():
    g = VG.grid_np(V.insert_np(cloud(), IDENT, VS), GRID, VS)
    s = S.surface_np(g.cls, g.top, SPRM)
    c = C.clearance_np(s.cls_out, CPRM)
    r = R.route_np(c.blocked, None, RPRM, np.array([GOAL], np.uint32), np.array([START], np.uint32))
    return {"grid": g, "surface": s, "clearance": c, "route": r,
            "way": G.waypoints_np(c.blocked, None, r.path, r.path_len, r.path_status, WPRM),
            "way_kept": G.waypoints_np(c.blocked, c.dist2, r.path, r.path_len, r.path_status, WPRM._replace(min_dist2=MIN_DIST2))}


def _facts(w):
    """w: what restated() gives, from the restatements or from the device"""
    g, c, r, way, kept = w["grid"], w["clearance"], w["route"], w["way"], w["way_kept"]
    gap = list(GAP)
    rows = np.arange(NA)
    assert (g.cls[~np.isin(rows, gap), WALL] == VG.OBSTACLE).all() and (g.cls[gap, WALL] == VG.LEVEL).all() and (g.cls[:, :WALL] == VG.LEVEL).all()
    open_rows = np.flatnonzero(c.blocked[:, WALL] == 0).tolist()
    assert open_rows == gap[1:-1]  # the inflation takes a row off either side
    m = int(r.path_len[0])
    cells = [divmod(int(v), NB) for v in r.path[0, :m]]
    assert r.path_status[0] == R.OK and cells[0] == divmod(START, NB) and cells[-1] == divmod(GOAL, NB) and any(b == WALL and a in open_rows for a, b in cells)
    # the waypoints: all of them written, none forced, far fewer than the path's cells
    n = int(way.way_len[0])
    assert way.way_status[0] == 0 and way.counts[4] == 0 and way.counts[:4] == (1, 0, m, n) and 3 <= n <= MAX_WAY and 4 * n < m
    ks = way.way_index[0, :n].tolist()
    assert ks[0] == 0 and ks[-1] == m - 1 and way.way[0, :n].tolist() == [int(r.path[0, k]) for k in ks]
    solid = lambda ia, ib: c.blocked[ia, ib] != 0
    assert all(G.clear_py(solid, cells[a], cells[b], MAX_LOOK) for a, b in zip(ks, ks[1:]))  # a host walk of every segment
    assert any(abs(cells[k][1] - WALL) <= 2 and cells[k][0] in gap for k in ks[1:-1])  # a waypoint lies at the gap
    stairs = 0.0
    for (a0, b0), (a1, b1) in zip(cells, cells[1:]):
        stairs += math.sqrt((a1 - a0) ** 2 + (b1 - b0) ** 2)
    assert 0.0 < float(way.length[0]) <= stairs * WPRM.cell_size  # the staircase in map units
    # with min_dist2: a segment that spans more than one path entry keeps the distance on every cell of its line, and a step between
    # neighbours is forced exactly where a cell the move touches is nearer than that
    near = lambda ia, ib: c.blocked[ia, ib] != 0 or int(c.dist2[ia, ib]) < MIN_DIST2
    n = int(kept.way_len[0])
    ks = kept.way_index[0, :n].tolist()
    forced = 0
    for a, b in zip(ks, ks[1:]):
        if b > a + 1:
            assert all(int(c.dist2[cell]) >= MIN_DIST2 for cell in G.line_py(*cells[a], *cells[b]))
        else:
            (a0, b0), (a1, b1) = cells[a], cells[b]
            forced += any(near(*cell) for cell in {(a0, b0), (a1, b1), (a1, b0), (a0, b1)})  # a diagonal move's side cells as well
    assert kept.way_status[0] == 0 and kept.counts[4] == forced and n >= int(way.way_len[0])
    # the route's own cells keep the distance, every one; what is forced are its diagonal moves past a nearer cell at the gap
    assert forced > 0 and all(int(c.dist2[cell]) >= MIN_DIST2 for cell in cells)


def test_the_restatements_show_the_wall_the_gap_and_the_way_through_it():
    w = restated()
    _facts(w)
    g = w["grid"]
    assert VG.same(g, VG.grid_py(V.insert_np(cloud(), IDENT, VS), GRID, VS))
    r = w["route"]
    assert G.same(w["way"], G.waypoints_py(w["clearance"].blocked, None, r.path, r.path_len, r.path_status, WPRM))
    print("path_len", r.path_len, "waypoints", w["way"].way_len, w["way"].way[0, :int(w["way"].way_len[0])], "kept", w["way_kept"].counts)


@pytest.mark.gpu
def test_grid_to_waypoints_on_the_stream_with_nothing_read_back(ctx):
    import torch
    import stereo_vo_amd as SV
    from stereo_vo_amd import api
    from test_grid_clearance import _api_params as clearance_params
    from test_grid_clearance import _eq as clearance_eq
    from test_grid_route import _api_params as route_params
    from test_grid_route import _eq as route_eq
    from test_grid_surface import _api_params as surface_params
    from test_grid_surface import _eq as surface_eq
    from test_grid_waypoints import _api_params as waypoint_params
    from test_voxel_grid import _eq as grid_eq
    n = NA * NB
    i32 = lambda count, fill: torch.full((count,), fill, dtype=torch.int32, device="cuda")
    u8 = lambda count, fill: torch.full((count,), fill, dtype=torch.uint8, device="cuda")
    i64 = lambda count, fill: torch.full((count,), fill, dtype=torch.int64, device="cuda")
    vm = SV.VoxelMap(ctx, voxel_size=VS, capacity_log2=LOG2, max_depth=0.0)
    pts = torch.from_numpy(np.ascontiguousarray(cloud()).view(np.int32).reshape(-1, 4).copy()).cuda()
    vm.insert(pts.data_ptr(), len(cloud()), m12=IDENT)
    gws, gcnt = i64(api.voxel_grid_workspace_bytes(NA, NB) // 8, 0x7F7F7F7F7F7F7F7F), i64(8, -1)
    cls, top, bottom, inten, nvox, npts = u8(n, 0xAA), i32(n, 0x5555AAAA), i32(n, 0x3333CCCC), u8(n, 0xBB), i32(n, 0x77777777), i64(n, 0x6666666666666666)
    cls_out, step, relief, support, scnt = u8(n, 0xBB), i32(n, 0x77777777), i32(n, 0x5555AAAA), torch.full((n,), 0x3333, dtype=torch.int16, device="cuda"), i64(8, -1)
    offsets, d2, near, clr, blk, ccnt = i32(n, 0x7F7F7F7F), i32(n, 0x5555AAAA), i32(n, 0x3333CCCC), i32(n, 0x77777777), u8(n, 0xBB), i64(8, -1)
    rws, cost, nxt = i64(api.grid_route_workspace_bytes(NA, NB) // 8, 0x7F7F7F7F7F7F7F7F), i32(n, 0x5555AAAA), u8(n, 0xBB)
    path, plen, status, rcnt = i32(MAX_PATH, 0x3333CCCC), i32(1, 0x77777777), u8(1, 0xEE), i64(8, -1)
    goals = torch.from_numpy(np.array([GOAL], np.uint32).view(np.int32)).cuda()
    starts = torch.from_numpy(np.array([START], np.uint32).view(np.int32)).cuda()
    outs = [dict(way=i32(MAX_WAY, -1), way_index=i32(MAX_WAY, -1), way_len=i32(1, 0x77771111), way_status=u8(1, 0xEE), length=i64(1, 0x5A5A5A5A5A5A5A5A),
                 counts=i64(8, -1)) for _ in range(2)]
    torch.cuda.synchronize()
    # the defaults for this route and this clearance, but the test's max_way
    wp = api.grid_waypoints_default_params(route_params(RPRM), clearance_params(CPRM))
    wp.max_way = MAX_WAY
    assert tuple(getattr(wp, f) for f in G.Params._fields) == tuple(WPRM)
    # everything from here to the sync is enqueued on the context's stream, each step reading the last one's device outputs
    vm.grid(api.VoxelGridParams(*GRID), workspace_ptr=gws.data_ptr(), cls_ptr=cls.data_ptr(), top_ptr=top.data_ptr(), bottom_ptr=bottom.data_ptr(),
            intensity_ptr=inten.data_ptr(), n_voxels_ptr=nvox.data_ptr(), n_points_ptr=npts.data_ptr(), counts_ptr=gcnt.data_ptr())
    ctx.grid_surface(cls.data_ptr(), top.data_ptr(), surface_params(SPRM), cls_out_ptr=cls_out.data_ptr(), step_ptr=step.data_ptr(),
                     relief_ptr=relief.data_ptr(), support_ptr=support.data_ptr(), counts_ptr=scnt.data_ptr())
    ctx.grid_clearance(cls_out.data_ptr(), clearance_params(CPRM), workspace_ptr=offsets.data_ptr(), dist2_ptr=d2.data_ptr(), nearest_ptr=near.data_ptr(),
                       clearance_ptr=clr.data_ptr(), blocked_ptr=blk.data_ptr(), counts_ptr=ccnt.data_ptr())
    ctx.grid_route(blk.data_ptr(), route_params(RPRM), goals.data_ptr(), 1, workspace_ptr=rws.data_ptr(), cost_ptr=cost.data_ptr(), next_ptr=nxt.data_ptr(),
                   starts_ptr=starts.data_ptr(), n_starts=1, path_ptr=path.data_ptr(), path_len_ptr=plen.data_ptr(), path_status_ptr=status.data_ptr(),
                   counts_ptr=rcnt.data_ptr())
    for o, (dist2_ptr, min_dist2) in zip(outs, ((None, 0), (d2.data_ptr(), MIN_DIST2))):
        ctx.grid_waypoints(blk.data_ptr(), path.data_ptr(), plen.data_ptr(), 1, waypoint_params(WPRM._replace(min_dist2=min_dist2)), dist2_ptr=dist2_ptr,
                           path_status_ptr=status.data_ptr(), **{k + "_ptr": t.data_ptr() for k, t in o.items()})
    ctx.sync()
    host = lambda t, kind=None, shape=(NA, NB): (t.cpu().numpy() if kind is None else t.cpu().numpy().view(kind)).reshape(shape)
    tally = lambda t, k: tuple(int(v) for v in t.cpu()[:k])
    got = {"grid": VG.Grid(host(cls), host(top, np.float32), host(bottom, np.float32), host(inten), host(nvox, np.uint32), host(npts, np.uint64), tally(gcnt, 5)),
           "surface": S.Surface(host(cls_out), host(step, np.float32), host(relief, np.float32), host(support, np.uint16), tally(scnt, 6)),
           "clearance": C.Clearance(host(d2, np.uint32), host(near, np.uint32), host(clr, np.float32), host(blk), tally(ccnt, 4)),
           "route": R.Route(host(cost, np.uint32), host(nxt), host(path, np.uint32, (1, MAX_PATH)), host(plen, np.uint32, (1,)), host(status, None, (1,)),
                            tally(rcnt, 6))}
    for name, o in zip(("way", "way_kept"), outs):
        assert int(o["counts"].cpu()[7]) == 0
        got[name] = G.Way(host(o["way"], np.uint32, (1, MAX_WAY)), host(o["way_index"], np.uint32, (1, MAX_WAY)), host(o["way_len"], np.uint32, (1,)),
                          host(o["way_status"], None, (1,)), host(o["length"], np.float64, (1,)), tally(o["counts"], 7))
    vm.close()
    w = restated()
    grid_eq(got["grid"], w["grid"])
    surface_eq(got["surface"], w["surface"])
    clearance_eq(got["clearance"], w["clearance"])
    route_eq(got["route"], w["route"], RPRM)
    for name in ("way", "way_kept"):
        print(name, "counts", got[name].counts, "way_len", got[name].way_len, "length", got[name].length, "path_len", got["route"].path_len)
        assert G.same(got[name], w[name]), (name, got[name], w[name])
    _facts(got)
