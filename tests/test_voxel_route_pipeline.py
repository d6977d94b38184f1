"""GPU: a pipeline's keyframe clouds fused into a voxel map, and a route through the map's free space from where the last keyframe's
camera stood (include/svo.h, "Voxel map route").  Three process calls with keyframe clouds on: every keyframe's cloud
is inserted under its pose7; then the occupancy volume is formed around the last pose, its distance field with the inflated volume,
and the route over `inflated` and `dist2` as they lie on the device, to the cell of the first keyframe's camera and to the volume's
last free cell, with paths from the last camera's cell and the first free cell.  Everything equals the restatement
(tests/voxel_route_ref.py) over the host copies of the two arrays.  Frame results, tracked set and clouds are byte-identical to a run
that never calls the entries."""
import numpy as np
import pytest

import voxel_rays_ref as R
import voxel_route_ref as V
from test_pipeline import _seq
from test_rectify import _bits, _params
from test_voxel_align_pipeline import _pose
from test_voxel_map_pipeline import DEPTH, H, LOG2, MD, VS, W, _bytes

pytestmark = pytest.mark.gpu
DIMS = (64, 32, 64)
MAX_DIST, RADIUS = 8, 0.3
NEAR_R2, NEAR_WEIGHT, MAX_PATH = 16, 4, 256


def test_a_route_from_the_camera_through_the_fused_map(ctx):
    import torch
    import stereo_vo_amd as S
    from stereo_vo_amd import api
    n, call = 12, 4
    p, Lt, Rt = _seq(n, w=W, h=H, seed=0x5EED0A00)
    pp = _params(S, p, MD)
    prm = api.CloudParams(2, 0.0, (W // 2) * (H // 2))
    cells = DIMS[0] * DIMS[1] * DIMS[2]

    def run(vm):
        pl = S.Pipeline(ctx, pp)
        pl.set_keyframe_clouds(prm)
        res, tabs, poses = [], [], []
        for b0 in range(0, n, call):
            res += pl.process_batch(Lt[b0:b0 + call], Rt[b0:b0 + call])
            tab = pl.keyframe_clouds()
            for t in tab if vm is not None else ():
                poses.append(_pose(b0 + t["frame"]))
                vm.insert(t["dev"], t["n_stored"], pose7=poses[-1])
            tabs += _bytes(tab)
        ids, xy = pl.tracked()
        pl.close()
        return [_bits(r) for r in res], tabs, (ids.tobytes(), xy.tobytes()), poses

    res0, tabs0, tracked0, _ = run(None)
    vm = S.VoxelMap(ctx, voxel_size=VS, capacity_log2=LOG2, max_depth=DEPTH)
    res1, tabs1, tracked1, poses = run(vm)
    assert len(poses) >= 2
    before = {k: v.copy() for k, v in vm.download().items()}
    centres = [api.pose7_to_cam_to_world(q).reshape(12)[[3, 7, 11]] for q in poses]
    origin = R.origin_of(tuple(centres[-1]), VS, DIMS)
    camera = api.voxel_occupancy_cell_of(VS, origin, DIMS, centres[-1])
    first = api.voxel_occupancy_cell_of(VS, origin, DIMS, centres[0])
    j = [int(np.floor(float(np.float32(x)) / float(np.float32(VS)))) - o for x, o in zip(centres[-1], origin)]
    assert camera == j[0] + DIMS[0] * (j[1] + DIMS[1] * j[2]) and all(abs(a - d // 2) <= 1 for a, d in zip(j, DIMS))  # centred on the last camera
    bits = torch.empty(cells // 64, dtype=torch.int64, device="cuda")
    occ = torch.zeros(2, dtype=torch.int32, device="cuda")
    dws = torch.full((api.voxel_distance_workspace_bytes(DIMS, False) // 8,), 0x5A5A, dtype=torch.int64, device="cuda")
    d2 = torch.full((cells,), 0x5555, dtype=torch.int16, device="cuda")
    infl = torch.full((cells // 64,), 0x5A5A, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    vm.occupancy(bits.data_ptr(), origin, DIMS, counts_ptr=occ.data_ptr())
    vm.distance(bits.data_ptr(), DIMS, workspace_ptr=dws.data_ptr(), dist2_ptr=d2.data_ptr(), inflated_ptr=infl.data_ptr(), max_dist=MAX_DIST, inflate_radius=RADIUS)
    ctx.sync()
    closed = V.unpack(infl.cpu().numpy().view(np.uint64), DIMS)
    dist2 = d2.cpu().numpy().view(np.uint16).reshape(closed.shape)
    free = np.flatnonzero(~closed.ravel())
    print("occupancy counts", occ.cpu().tolist(), "closed after inflation", int(closed.sum()), "camera cell", camera, "first keyframe's", first)
    assert int(occ[0]) > 0 and closed.sum() > int(occ[0]) and len(free) > cells // 2
    goals = np.array([first, free[-1]], np.uint32)
    starts = np.array([camera, free[0], cells], np.uint32)
    case = V.Case(closed, dist2, V.params(NEAR_R2, NEAR_WEIGHT, max_path=MAX_PATH), goals, starts)
    want = V.route_np(*case)
    rounds = want.sweeps + 2
    print("route counts", want.counts, "sweeps", want.sweeps, "path_len", want.path_len, "status", want.path_status)
    assert want.counts[0] >= 1 and want.path_status[2] == V.OUT_OF_VOLUME
    # the device entry, over the arrays where the distance field left them
    gt = torch.from_numpy(goals.view(np.int32).copy()).cuda()
    st = torch.from_numpy(starts.view(np.int32).copy()).cuda()
    ws = torch.full((api.voxel_route_workspace_bytes(DIMS) // 8,), 0x5A5A, dtype=torch.int64, device="cuda")
    cost = torch.full((cells,), -2, dtype=torch.int32, device="cuda")
    nxt = torch.full((cells,), 0x5A, dtype=torch.uint8, device="cuda")
    path = torch.full((len(starts) * MAX_PATH,), -2, dtype=torch.int32, device="cuda")
    plen = torch.full((len(starts),), -2, dtype=torch.int32, device="cuda")
    pst = torch.full((len(starts),), 0x5A, dtype=torch.uint8, device="cuda")
    cnt = torch.full((8,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    vm.route(infl.data_ptr(), DIMS, gt.data_ptr(), len(goals), dist2_ptr=d2.data_ptr(), starts_ptr=st.data_ptr(), n_starts=len(starts), workspace_ptr=ws.data_ptr(),
             cost_ptr=cost.data_ptr(), next_ptr=nxt.data_ptr(), path_ptr=path.data_ptr(), path_len_ptr=plen.data_ptr(), path_status_ptr=pst.data_ptr(),
             counts_ptr=cnt.data_ptr(), near_r2=NEAR_R2, near_weight=NEAR_WEIGHT, max_path=MAX_PATH, max_rounds=rounds)
    ctx.sync()
    c = cnt.cpu().tolist()
    assert tuple(c[:5]) == want.counts and 0 <= c[5] <= rounds and c[6:] == [0, 0]
    assert np.array_equal(cost.cpu().numpy().view(np.uint32).reshape(closed.shape), want.cost) and np.array_equal(nxt.cpu().numpy().reshape(closed.shape), want.next)
    assert np.array_equal(plen.cpu().numpy().view(np.uint32), want.path_len) and np.array_equal(pst.cpu().numpy(), want.path_status)
    got_path = path.cpu().numpy().view(np.uint32).reshape(len(starts), MAX_PATH)
    written = np.arange(MAX_PATH)[None, :] < np.minimum(want.path_len, MAX_PATH)[:, None]
    assert np.array_equal(got_path[written], want.path[written]) and (got_path[~written] == 0xFFFFFFFE).all()
    assert np.array_equal(infl.cpu().numpy().view(np.uint64), V.pack(closed)) and np.array_equal(d2.cpu().numpy().view(np.uint16), dist2.ravel())  # only read
    # the host entry
    h = vm.route_host(infl.data_ptr(), DIMS, goals, starts=starts, dist2_ptr=d2.data_ptr(), near_r2=NEAR_R2, near_weight=NEAR_WEIGHT, max_path=MAX_PATH, max_rounds=rounds)
    assert np.array_equal(h["cost"], want.cost) and np.array_equal(h["next"], want.next) and np.array_equal(h["path"], want.path)
    assert np.array_equal(h["path_len"], want.path_len) and tuple(h["counts"][k] for k in api.VOXEL_ROUTE_COUNTS[:5]) == want.counts
    after = vm.download()
    assert all(np.array_equal(before[k], after[k]) for k in before)  # nothing of this changes the map
    assert res1 == res0 and tabs1 == tabs0 and tracked1 == tracked0
    vm.close()
