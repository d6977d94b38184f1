"""GPU: the route over the clearance of a voxel map's ground plan, the map filled from the keyframe clouds of a pipeline and of a
two-lane pipeline group (include/svo.h, "Ground plan route").  After every one of three process calls the call's clouds
are inserted under their frame's pose7, the grid is built, its clearance is computed with an inflation and the route is computed from
the clearance's DEVICE blocked and dist2, all on the context's stream.  Every route equals the restatement (tests/grid_route_ref.py)
over the host copies of those two arrays; computing it changes no bit of the frame results, the tracked set, the clouds, the grids or
the clearances of a run that never calls the entry."""
import numpy as np
import pytest

import grid_route_ref as G
from test_grid_route import _api_params, _bounded, _eq
from test_pipeline import _seq
from test_rectify import _bits, _params
from test_voxel_grid_pipeline import PARAMS
from test_voxel_map_pipeline import DEPTH, H, LOG2, MD, VS, W, _bytes, _pose

pytestmark = pytest.mark.gpu

MASK = 1 << 1 | 1 << 2  # LEVEL and OBSTACLE: every cell the map has a surface in
MAX_DIST, RADIUS = 6, 0.7  # cells of 0.6: the cells beside a surface are inside the inflation
NEAR_R2, NEAR_WEIGHT, MAX_PATH = 16, 4, 40


def _grid_clearance_then_route(ctx, vm, route):
    """The grid's cls and the clearance's dist2 and blocked as bytes and, with `route`, (the case, its restatement, the device's G.Route)."""
    import torch
    from stereo_vo_amd import api
    gp = api.VoxelGridParams(*PARAMS)
    na, nb = gp.na, gp.nb
    n = na * nb
    ws = torch.empty(4 * n, dtype=torch.int64, device="cuda")
    cls = torch.full((n,), 0xAA, dtype=torch.uint8, device="cuda")
    offsets = torch.full((n,), 0x7F7F7F7F, dtype=torch.int32, device="cuda")
    d2 = torch.full((n,), 0x5555AAAA, dtype=torch.int32, device="cuda")
    blk = torch.full((n,), 0xBB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    vm.grid(gp, workspace_ptr=ws.data_ptr(), cls_ptr=cls.data_ptr())
    cp = api.grid_clearance_default_params(gp, VS)
    cp.source_mask, cp.max_dist, cp.inflate_radius = MASK, MAX_DIST, RADIUS
    ctx.grid_clearance(cls.data_ptr(), cp, workspace_ptr=offsets.data_ptr(), dist2_ptr=d2.data_ptr(), blocked_ptr=blk.data_ptr())
    ctx.sync()
    h_d2, h_blk = d2.cpu().numpy().view(np.uint32).reshape(na, nb), blk.cpu().numpy().reshape(na, nb)
    state = (cls.cpu().numpy().tobytes(), h_d2.tobytes(), h_blk.tobytes())
    if not route:
        return state, None
    rp = api.grid_route_default_params(cp)
    assert (rp.na, rp.nb, rp.max_rounds, rp.max_cost) == (na, nb, 64, api.GRID_ROUTE_MAX_COST)
    prm = G.Params(na, nb, NEAR_R2, NEAR_WEIGHT, rp.max_cost, rp.max_rounds, MAX_PATH, 0)
    corners = [0, nb - 1, (na - 1) * nb, n - 1]
    case, w = _bounded(G.Case(h_blk, h_d2, prm, np.array([(na // 2) * nb + nb // 2] + corners, np.uint32),
                              np.array(corners + [(na // 4) * nb + nb // 4, n], np.uint32)))
    ns = len(case.starts)
    goals, starts = (torch.from_numpy(np.asarray(a, np.uint32).view(np.int32)).cuda() for a in (case.goals, case.starts))
    rws = torch.full((api.grid_route_workspace_bytes(na, nb) // 8,), 0x7F7F7F7F7F7F7F7F, dtype=torch.int64, device="cuda")
    cost = torch.full((n,), 0x5555AAAA, dtype=torch.int32, device="cuda")
    nxt = torch.full((n,), 0xBB, dtype=torch.uint8, device="cuda")
    path = torch.full((ns * MAX_PATH,), 0x3333CCCC, dtype=torch.int32, device="cuda")
    plen = torch.full((ns,), 0x77777777, dtype=torch.int32, device="cuda")
    status = torch.full((ns,), 0xEE, dtype=torch.uint8, device="cuda")
    cnt = torch.full((8,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.grid_route(blk.data_ptr(), _api_params(case.prm), goals.data_ptr(), len(case.goals), workspace_ptr=rws.data_ptr(), cost_ptr=cost.data_ptr(),
                   dist2_ptr=d2.data_ptr(), next_ptr=nxt.data_ptr(), starts_ptr=starts.data_ptr(), n_starts=ns, path_ptr=path.data_ptr(),
                   path_len_ptr=plen.data_ptr(), path_status_ptr=status.data_ptr(), counts_ptr=cnt.data_ptr())
    ctx.sync()
    u32 = lambda t: t.cpu().numpy().view(np.uint32)
    got = G.Route(u32(cost).reshape(na, nb), nxt.cpu().numpy().reshape(na, nb), u32(path).reshape(ns, MAX_PATH), u32(plen), status.cpu().numpy(),
                  tuple(int(v) for v in cnt.cpu()[:6]))
    # the route only read what the clearance left
    assert (cls.cpu().numpy().tobytes(), d2.cpu().numpy().tobytes(), blk.cpu().numpy().tobytes()) == state
    return state, (case, w, got)


def _check(results):
    seen = []
    for case, w, got in results:
        print("route counts (n_goals_used, n_reached, n_unreached, n_impassable, converged), rounds:", w.counts, got.counts[5], "of", case.prm.max_rounds)
        assert w.counts[0] >= 1 and w.counts[1] >= 100 and w.counts[3] >= 1 and sum(w.counts[1:4]) == case.prm.na * case.prm.nb
        assert (w.path_status == G.OUT_OF_GRID).sum() == 1 and (w.path_status <= G.TRUNCATED).sum() >= 1
        _eq(got, w, case.prm)
        seen.append(w.counts)
    return seen


def test_pipeline_keyframe_clouds_into_a_grid_its_clearance_and_the_route(ctx):
    import stereo_vo_amd as S
    from stereo_vo_amd import api
    n, call = 12, 4
    p, L, R = _seq(n, w=W, h=H, seed=0x5EED0A00)
    pp = _params(S, p, MD)
    prm = api.CloudParams(2, 0.0, (W // 2) * (H // 2))

    def run(route):
        vm = S.VoxelMap(ctx, voxel_size=VS, capacity_log2=LOG2, max_depth=DEPTH)
        pl = S.Pipeline(ctx, pp)
        pl.set_keyframe_clouds(prm)
        res, tabs, states, results = [], [], [], []
        for b0 in range(0, n, call):
            res += pl.process_batch(L[b0:b0 + call], R[b0:b0 + call])
            tab = pl.keyframe_clouds()
            tabs += _bytes(tab)
            vm.insert_keyframe_clouds(tab, [_pose(0, b0 + t["frame"]) for t in tab])  # before the next call replaces the clouds
            s, r = _grid_clearance_then_route(ctx, vm, route)
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
    assert len(set(_check(results))) >= 2  # the map grew between the routes


def test_group_of_two_lanes_one_map_and_one_route_per_lane(ctx):
    import stereo_vo_amd as S
    from stereo_vo_amd import api
    lanes, batch, calls = 2, 2, 3
    n = batch * calls
    seqs = [_seq(n, w=W, h=H, seed=0x5EED0A00 + 17 * i) for i in range(lanes)]
    pp = _params(S, seqs[0][0], MD)
    Ls, Rs = np.stack([s[1] for s in seqs]), np.stack([s[2] for s in seqs])
    prm = api.CloudParams(2, 0.0, (W // 2) * (H // 2))

    def run(route):
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
                s, got = _grid_clearance_then_route(ctx, maps[l], route)
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
