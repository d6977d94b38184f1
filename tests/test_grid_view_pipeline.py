"""GPU: the planning cycle of tests/test_grid_frontier_pipeline.py with the view as its fifth step (include/svo.h, "Ground plan view";
INTEGRATION 4a), over a voxel map filled from the keyframe clouds of a pipeline and of a two-lane pipeline group.  After every one of
three process calls the call's clouds are inserted under their frame's pose7, the grid is built, its clearance is computed with an
inflation, a first route is computed whose only goal is the vehicle's cell, the frontiers are computed from the DEVICE cls, blocked and
that cost, the view is computed over the frontiers' DEVICE goal_cells with n_views = max_frontiers = 64 and the first route's DEVICE
cost, and a second route takes the view's DEVICE best with n_goals = 1 and a start at the vehicle's cell: nothing is read back in
between.  The view equals the restatement (tests/grid_view_ref.py) over the host copies of its three inputs and the second route equals
tests/grid_route_ref.py over the host copy of best[0]; the cycle changes no bit of the frame results, the tracked set, the clouds, the
grids, the clearances, the first routes or the frontiers of a run that never calls the entry."""
import numpy as np
import pytest

import grid_frontier_ref as F
import grid_route_ref as G
import grid_view_ref as V
from test_grid_frontier import _api_params as _frontier_params
from test_grid_frontier_pipeline import MAX_DIST, MAX_FRONTIERS, MAX_PATH, MIN_SIZE, RADIUS, ROUNDS
from test_grid_route import _api_params as _route_params
from test_grid_route import _eq as _route_eq
from test_grid_view import _api_params as _view_params
from test_grid_view import _eq as _view_eq
from test_pipeline import _seq
from test_rectify import _bits, _params
from test_voxel_grid_pipeline import PARAMS
from test_voxel_map_pipeline import DEPTH, H, LOG2, MD, VS, W, _bytes, _pose

pytestmark = pytest.mark.gpu

MAX_RANGE = 12  # cells of 0.6 on a 50 x 50 plan


def _cycle(ctx, vm, view):
    """(cls, dist2, blocked, the first route's cost, the frontiers' records, goal_cells and label as bytes; with `view`, what the view and
    the second route gave and should)"""
    import torch
    from stereo_vo_amd import api
    gp = api.VoxelGridParams(*PARAMS)
    na, nb = gp.na, gp.nb
    n = na * nb
    vehicle = (na // 2) * nb + nb // 2
    i32 = lambda count, fill: torch.full((count,), fill, dtype=torch.int32, device="cuda")
    u8 = lambda count, fill: torch.full((count,), fill, dtype=torch.uint8, device="cuda")
    i64 = lambda count, fill: torch.full((count,), fill, dtype=torch.int64, device="cuda")
    ws = torch.empty(4 * n, dtype=torch.int64, device="cuda")
    cls, offsets, d2, blk = u8(n, 0xAA), i32(n, 0x7F7F7F7F), i32(n, 0x5555AAAA), u8(n, 0xBB)
    rws = [i64(api.grid_route_workspace_bytes(na, nb) // 8, 0x7F7F7F7F7F7F7F7F) for _ in range(2)]
    cost = [i32(n, 0x5555AAAA) for _ in range(2)]
    here = torch.from_numpy(np.array([vehicle], np.uint32).view(np.int32)).cuda()
    fws = i64(api.grid_frontier_workspace_bytes(na, nb, MAX_FRONTIERS) // 8, 0x7F7F7F7F7F7F7F7F)
    frec, goal, label = i64(6 * MAX_FRONTIERS, 0x5A5A5A5A5A5A5A5A), i32(MAX_FRONTIERS, 0x3333CCCC), i32(n, 0x5555AAAA)
    vws = i64(api.grid_view_workspace_bytes(na, nb, MAX_FRONTIERS) // 8, 0x7F7F7F7F7F7F7F7F)
    vrec, order, best, seen = i64(4 * MAX_FRONTIERS, 0x5A5A5A5A5A5A5A5A), i32(MAX_FRONTIERS, 0x3333CCCC), i32(4, 0x77771111), i32(n, 0x5555AAAA)
    vcnt, rcnt = (i64(8, -1) for _ in range(2))
    nxt, path, plen, status = u8(n, 0xBB), i32(MAX_PATH, 0x3333CCCC), i32(1, 0x77777777), u8(1, 0xEE)
    torch.cuda.synchronize()
    cp = api.grid_clearance_default_params(gp, VS)
    cp.max_dist, cp.inflate_radius = MAX_DIST, RADIUS
    rprm = G.Params(na, nb, 0, 0, G.MAX_COST, ROUNDS, MAX_PATH, 0)
    fprm = F.Params(na, nb, 1 << F.LEVEL, 1 << F.UNKNOWN, MIN_SIZE, MAX_FRONTIERS)
    vprm = V.Params(na, nb, 1 << V.OBSTACLE, 1 << V.UNKNOWN, MAX_RANGE, 16, 1)
    # everything from here to the sync is enqueued on the context's stream, each step reading the last one's device outputs
    vm.grid(gp, workspace_ptr=ws.data_ptr(), cls_ptr=cls.data_ptr())
    ctx.grid_clearance(cls.data_ptr(), cp, workspace_ptr=offsets.data_ptr(), dist2_ptr=d2.data_ptr(), blocked_ptr=blk.data_ptr())
    ctx.grid_route(blk.data_ptr(), _route_params(rprm), here.data_ptr(), 1, workspace_ptr=rws[0].data_ptr(), cost_ptr=cost[0].data_ptr())
    ctx.grid_frontiers(cls.data_ptr(), _frontier_params(fprm), blocked_ptr=blk.data_ptr(), cost_ptr=cost[0].data_ptr(), workspace_ptr=fws.data_ptr(),
                       frontiers_ptr=frec.data_ptr(), goal_cells_ptr=goal.data_ptr(), label_ptr=label.data_ptr())
    if view:
        ctx.grid_view(cls.data_ptr(), goal.data_ptr(), MAX_FRONTIERS, _view_params(vprm), cost_ptr=cost[0].data_ptr(), workspace_ptr=vws.data_ptr(),
                      records_ptr=vrec.data_ptr(), order_ptr=order.data_ptr(), best_ptr=best.data_ptr(), seen_ptr=seen.data_ptr(), counts_ptr=vcnt.data_ptr())
        ctx.grid_route(blk.data_ptr(), _route_params(rprm), best.data_ptr(), 1, workspace_ptr=rws[1].data_ptr(), cost_ptr=cost[1].data_ptr(),
                       next_ptr=nxt.data_ptr(), starts_ptr=here.data_ptr(), n_starts=1, path_ptr=path.data_ptr(), path_len_ptr=plen.data_ptr(),
                       path_status_ptr=status.data_ptr(), counts_ptr=rcnt.data_ptr())
    ctx.sync()
    u32 = lambda t: t.cpu().numpy().view(np.uint32)
    h_cls, h_cost, h_goal = cls.cpu().numpy().reshape(na, nb), u32(cost[0]).reshape(na, nb), u32(goal)
    state = (h_cls.tobytes(), u32(d2).tobytes(), blk.cpu().numpy().tobytes(), h_cost.tobytes(), frec.cpu().numpy().tobytes(), h_goal.tobytes(),
             u32(label).tobytes())
    if not view:
        return state, None
    vgot = {"records": vrec.cpu().numpy().view(V.RECORD), "order": u32(order), "best": u32(best), "seen": u32(seen).reshape(na, nb),
            "counts": tuple(int(v) for v in vcnt.cpu())}
    vwant = V.views_np(h_cls, h_goal, h_cost, vprm)
    assert V.same(vwant, V.views_py(h_cls, h_goal, h_cost, vprm))
    rgot = G.Route(u32(cost[1]).reshape(na, nb), nxt.cpu().numpy().reshape(na, nb), u32(path).reshape(1, MAX_PATH), u32(plen), status.cpu().numpy(),
                   tuple(int(v) for v in rcnt.cpu()[:6]))
    rwant = G.route_np(blk.cpu().numpy().reshape(na, nb), None, rprm, vgot["best"][:1], np.array([vehicle], np.uint32))
    return state, (vgot, vwant, rgot, rwant, rprm)


def _check(results):
    seen = []
    for vgot, vwant, rgot, rwant, rprm in results:
        print("view counts", vwant.counts, "best", vwant.best.tolist(), "second route counts", rwant.counts, "status", rwant.path_status, "len", rwant.path_len)
        _view_eq(vgot, vwant)
        _route_eq(rgot, rwant, rprm)
        # the cycle has something to choose from: used views beside the padding.  Where a view is worth its way the second route goes to
        # it; where none is (the vehicle's cell is inside the inflation, so nothing has a way there) best is the NONE record, which the
        # second route ignores
        assert vwant.counts[0] >= 1 and vwant.counts[1] >= 1 and vwant.counts[0] + vwant.counts[1] == MAX_FRONTIERS and rwant.counts[4] == 1
        if vwant.best[2] > 0:
            assert vwant.best[3] > 0 and vwant.best[0] == vwant.records[vwant.best[1]]["cell"] and rwant.counts[0] == 1
        else:
            assert vwant.best.tolist() == [V.NONE, V.NONE, 0, 0] and rwant.counts[0] == 0 and (vwant.records["score"] == 0).all()
        seen.append(tuple(vwant.counts) + tuple(vwant.best.tolist()))
    return seen


def test_pipeline_keyframe_clouds_into_one_planning_cycle_with_a_view(ctx):
    import stereo_vo_amd as S
    from stereo_vo_amd import api
    n, call = 12, 4
    p, L, R = _seq(n, w=W, h=H, seed=0x5EED0A00)
    pp = _params(S, p, MD)
    prm = api.CloudParams(2, 0.0, (W // 2) * (H // 2))

    def run(view):
        vm = S.VoxelMap(ctx, voxel_size=VS, capacity_log2=LOG2, max_depth=DEPTH)
        pl = S.Pipeline(ctx, pp)
        pl.set_keyframe_clouds(prm)
        res, tabs, states, results = [], [], [], []
        for b0 in range(0, n, call):
            res += pl.process_batch(L[b0:b0 + call], R[b0:b0 + call])
            tab = pl.keyframe_clouds()
            tabs += _bytes(tab)
            vm.insert_keyframe_clouds(tab, [_pose(0, b0 + t["frame"]) for t in tab])  # before the next call replaces the clouds
            s, r = _cycle(ctx, vm, view)
            states.append(s)
            results.append(r)
        ids, xy = pl.tracked()
        pl.close()
        vm.close()
        return [_bits(r) for r in res], tabs, (ids.tobytes(), xy.tobytes()), states, results

    res0, tabs0, tracked0, states0, _ = run(False)
    res1, tabs1, tracked1, states1, results = run(True)
    assert res1 == res0 and tabs1 == tabs0 and tracked1 == tracked0 and states1 == states0
    assert len(results) == 3  # one per process call
    seen = _check(results)
    assert len(set(seen)) >= 2  # the map grew between the cycles
    assert any(s[-2] > 0 for s in seen)  # a goal was chosen in one cycle at least


def test_group_of_two_lanes_one_map_and_one_planning_cycle_with_a_view_per_lane(ctx):
    import stereo_vo_amd as S
    from stereo_vo_amd import api
    lanes, batch, calls = 2, 2, 3
    n = batch * calls
    seqs = [_seq(n, w=W, h=H, seed=0x5EED0A00 + 17 * i) for i in range(lanes)]
    pp = _params(S, seqs[0][0], MD)
    Ls, Rs = np.stack([s[1] for s in seqs]), np.stack([s[2] for s in seqs])
    prm = api.CloudParams(2, 0.0, (W // 2) * (H // 2))

    def run(view):
        maps = [S.VoxelMap(ctx, voxel_size=VS, capacity_log2=LOG2, max_depth=DEPTH) for _ in range(lanes)]
        g = S.PipelineGroup(ctx, pp, lanes)
        g.set_keyframe_clouds(-1, prm)
        res, tabs, states, results = [[] for _ in range(lanes)], [], [], [[] for _ in range(lanes)]
        for b0 in range(0, n, batch):
            r = g.process_batch(Ls[:, b0:b0 + batch], Rs[:, b0:b0 + batch])
            tab = g.keyframe_clouds()
            tabs += _bytes(tab)
            for l in range(lanes):
                res[l] += [_bits(x) for x in r[l]]
                mine = [t for t in tab if t["lane"] == l]
                maps[l].insert_keyframe_clouds(mine, [_pose(l, b0 + t["frame"]) for t in mine])
                s, got = _cycle(ctx, maps[l], view)
                states.append(s)
                results[l].append(got)
        g.close()
        for vm in maps:
            vm.close()
        return res, tabs, states, results

    res0, tabs0, states0, _ = run(False)
    res1, tabs1, states1, results = run(True)
    assert res1 == res0 and tabs1 == tabs0 and states1 == states0
    seen = [_check(r) for r in results]
    assert all(len(s) == calls for s in seen) and seen[0] != seen[1]  # the lanes' maps differ
    assert any(s[-2] > 0 for lane in seen for s in lane)  # a goal was chosen in one cycle at least
