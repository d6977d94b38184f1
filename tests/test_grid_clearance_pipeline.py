"""GPU: the clearance of a voxel map's ground plan, the map filled from the keyframe clouds of a pipeline and of a two-lane pipeline
group (include/svo.h, "Ground plan clearance").  After every one of three process calls the call's clouds are inserted
under their frame's pose7, the grid is built and the clearance is computed from the grid's DEVICE cls, all on the context's stream.
Every clearance equals the restatement (tests/grid_clearance_ref.py) over the host copy of that cls; computing it changes no bit of the
frame results, the tracked set, the clouds or the grids of a run that never calls the entry."""
import numpy as np
import pytest

import grid_clearance_ref as G
from test_grid_clearance import _eq
from test_pipeline import _seq
from test_rectify import _bits, _params
from test_voxel_grid_pipeline import PARAMS
from test_voxel_map_pipeline import DEPTH, H, LOG2, MD, VS, W, _bytes, _pose

pytestmark = pytest.mark.gpu

MASK = 1 << 1 | 1 << 2  # LEVEL and OBSTACLE: every cell the map has a surface in
MAX_DIST, RADIUS = 6, 1.3


def _grid_then_clearance(ctx, vm, clearance):
    """The grid's cls as bytes and, with `clearance`, (host cls, the parameters, the G.Clearance the device gave)."""
    import torch
    from stereo_vo_amd import api
    gp = api.VoxelGridParams(*PARAMS)
    n = gp.na * gp.nb
    ws = torch.empty(4 * n, dtype=torch.int64, device="cuda")
    cls = torch.full((n,), 0xAA, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    vm.grid(gp, workspace_ptr=ws.data_ptr(), cls_ptr=cls.data_ptr())
    got = None
    if clearance:
        cp = api.grid_clearance_default_params(gp, VS)
        assert (cp.na, cp.nb, cp.cell_size, cp.source_mask) == (gp.na, gp.nb, gp.cell_voxels * float(np.float32(VS)), 1 << 2)
        cp.source_mask, cp.max_dist, cp.inflate_radius = MASK, MAX_DIST, RADIUS
        offsets = torch.full((n,), 0x7F7F7F7F, dtype=torch.int32, device="cuda")
        d2, near, clr = (torch.full((n,), 0x5555AAAA, dtype=torch.int32, device="cuda") for _ in range(3))
        blk = torch.full((n,), 0xBB, dtype=torch.uint8, device="cuda")
        cnt = torch.full((4,), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ctx.grid_clearance(cls.data_ptr(), cp, workspace_ptr=offsets.data_ptr(), dist2_ptr=d2.data_ptr(), nearest_ptr=near.data_ptr(),
                           clearance_ptr=clr.data_ptr(), blocked_ptr=blk.data_ptr(), counts_ptr=cnt.data_ptr())
        ctx.sync()
        shape = (gp.na, gp.nb)
        got = (G.Params(cp.na, cp.nb, cp.source_mask, cp.max_dist, cp.cell_size, cp.inflate_radius),
               G.Clearance(d2.cpu().numpy().view(np.uint32).reshape(shape), near.cpu().numpy().view(np.uint32).reshape(shape),
                           clr.cpu().numpy().view(np.float32).reshape(shape), blk.cpu().numpy().reshape(shape), tuple(int(v) for v in cnt.cpu())))
    ctx.sync()
    host = cls.cpu().numpy().reshape(gp.na, gp.nb)
    return host.tobytes(), None if got is None else (host,) + got


def _check(results):
    seen = []
    for host, prm, got in results:
        w = G.clearance_np(host, prm)
        print("clearance counts (n_sources, n_reached, n_unreached, n_blocked):", w.counts)
        assert w.counts[0] >= 1 and w.counts[1] >= 1 and w.counts[3] >= 1 and sum(w.counts[:3]) == prm.na * prm.nb
        _eq(got, w)
        seen.append(w.counts)
    return seen


def test_pipeline_keyframe_clouds_into_a_grid_and_its_clearance(ctx):
    import stereo_vo_amd as S
    from stereo_vo_amd import api
    n, call = 12, 4
    p, L, R = _seq(n, w=W, h=H, seed=0x5EED0A00)
    pp = _params(S, p, MD)
    prm = api.CloudParams(2, 0.0, (W // 2) * (H // 2))

    def run(clearance):
        vm = S.VoxelMap(ctx, voxel_size=VS, capacity_log2=LOG2, max_depth=DEPTH)
        pl = S.Pipeline(ctx, pp)
        pl.set_keyframe_clouds(prm)
        res, tabs, grids, results = [], [], [], []
        for b0 in range(0, n, call):
            res += pl.process_batch(L[b0:b0 + call], R[b0:b0 + call])
            tab = pl.keyframe_clouds()
            tabs += _bytes(tab)
            vm.insert_keyframe_clouds(tab, [_pose(0, b0 + t["frame"]) for t in tab])  # before the next call replaces the clouds
            g, r = _grid_then_clearance(ctx, vm, clearance)
            grids.append(g)
            results.append(r)
        ids, xy = pl.tracked()
        pl.close()
        vm.close()
        return [_bits(r) for r in res], tabs, (ids.tobytes(), xy.tobytes()), grids, results

    res0, tabs0, tracked0, grids0, _ = run(False)
    res1, tabs1, tracked1, grids1, results = run(True)
    assert res1 == res0 and tabs1 == tabs0 and tracked1 == tracked0 and grids1 == grids0
    assert len(results) == 3  # one per process call
    assert len(set(_check(results))) >= 2  # the map grew between the grids


def test_group_of_two_lanes_one_map_and_one_clearance_per_lane(ctx):
    import stereo_vo_amd as S
    from stereo_vo_amd import api
    lanes, batch, calls = 2, 2, 3
    n = batch * calls
    seqs = [_seq(n, w=W, h=H, seed=0x5EED0A00 + 17 * i) for i in range(lanes)]
    pp = _params(S, seqs[0][0], MD)
    Ls, Rs = np.stack([s[1] for s in seqs]), np.stack([s[2] for s in seqs])
    prm = api.CloudParams(2, 0.0, (W // 2) * (H // 2))

    def run(clearance):
        maps = [S.VoxelMap(ctx, voxel_size=VS, capacity_log2=LOG2, max_depth=DEPTH) for _ in range(lanes)]
        g = S.PipelineGroup(ctx, pp, lanes)
        g.set_keyframe_clouds(-1, prm)
        res, tabs, grids, results = [[] for _ in range(lanes)], [], [], [[] for _ in range(lanes)]
        for b0 in range(0, n, batch):
            r = g.process_batch(Ls[:, b0:b0 + batch], Rs[:, b0:b0 + batch])
            tab = g.keyframe_clouds()
            tabs += _bytes(tab)
            for l in range(lanes):
                res[l] += [_bits(x) for x in r[l]]
                mine = [t for t in tab if t["lane"] == l]
                maps[l].insert_keyframe_clouds(mine, [_pose(l, b0 + t["frame"]) for t in mine])
                grid, got = _grid_then_clearance(ctx, maps[l], clearance)
                grids.append(grid)
                results[l].append(got)
        g.close()
        for vm in maps:
            vm.close()
        return res, tabs, grids, results

    res0, tabs0, grids0, _ = run(False)
    res1, tabs1, grids1, results = run(True)
    assert res1 == res0 and tabs1 == tabs0 and grids1 == grids0
    seen = [_check(r) for r in results]
    assert all(len(s) == calls for s in seen) and seen[0] != seen[1]  # the lanes' maps differ
