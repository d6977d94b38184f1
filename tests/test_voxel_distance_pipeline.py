"""GPU: a pipeline's keyframe clouds fused into a voxel map, and the map's distance field asked where the keyframes' cameras stood
(include/svo.h, "Voxel map distance field").  Three process calls with keyframe clouds on: every keyframe's cloud is
inserted under its pose7; then the occupancy volume is formed around the last pose, its distance field with every output, and the
keyframes' camera centres are queried as spheres.  Everything equals the restatement (tests/voxel_distance_ref.py) over the host
copy of the bits.  Frame results, tracked set and clouds are byte-identical to a run that never calls the entries."""
import numpy as np
import pytest

import voxel_distance_ref as D
import voxel_rays_ref as R
from test_pipeline import _seq
from test_rectify import _bits, _params
from test_voxel_align_pipeline import _pose
from test_voxel_map_pipeline import DEPTH, H, LOG2, MD, VS, W, _bytes

pytestmark = pytest.mark.gpu
DIMS = (128, 64, 128)
MAX_DIST, RADIUS = 8, 0.3


def test_the_distance_field_of_the_fused_map_and_the_camera_centres_in_it(ctx):
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
    bits = torch.empty(cells // 64, dtype=torch.int64, device="cuda")
    occ = torch.zeros(2, dtype=torch.int32, device="cuda")
    ws = torch.full((api.voxel_distance_workspace_bytes(DIMS, True) // 8,), 0x5A5A, dtype=torch.int64, device="cuda")
    d2 = torch.full((cells,), 0x5555, dtype=torch.int16, device="cuda")
    near = torch.full((cells,), -2, dtype=torch.int32, device="cuda")
    clr = torch.full((cells,), -2, dtype=torch.int32, device="cuda")
    infl = torch.full((cells // 64,), 0x5A5A, dtype=torch.int64, device="cuda")
    cnt = torch.full((4,), -1, dtype=torch.int64, device="cuda")
    spheres = np.zeros(len(centres), api.VoxelSphere)
    for i, c in enumerate(centres):
        spheres[i] = (*c.astype(np.float32), RADIUS)
    st = torch.from_numpy(spheres.view(np.int32).reshape(-1, 4).copy()).cuda()
    hits = torch.full((4 * len(centres),), -1, dtype=torch.int32, device="cuda")
    qcnt = torch.full((6,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    vm.occupancy(bits.data_ptr(), origin, DIMS, counts_ptr=occ.data_ptr())
    vm.distance(bits.data_ptr(), DIMS, workspace_ptr=ws.data_ptr(), dist2_ptr=d2.data_ptr(), nearest_ptr=near.data_ptr(), clearance_ptr=clr.data_ptr(),
                inflated_ptr=infl.data_ptr(), counts_ptr=cnt.data_ptr(), max_dist=MAX_DIST, inflate_radius=RADIUS)
    vm.distance_query(d2.data_ptr(), origin, DIMS, st.data_ptr(), len(centres), hits_ptr=hits.data_ptr(), counts_ptr=qcnt.data_ptr())
    ctx.sync()
    words = bits.cpu().numpy().view(np.uint64)
    want = D.field(words, DIMS, MAX_DIST, RADIUS, VS)
    print("distance counts (n_sources, n_reached, n_unreached, n_inflated):", want["counts"], "R2", want["r2"])
    assert want["counts"][0] == int(occ[0]) > 100 and want["counts"][3] > want["counts"][0]
    assert np.array_equal(d2.cpu().numpy().view(np.uint16), want["dist2"]) and np.array_equal(near.cpu().numpy().view(np.uint32), want["nearest"])
    assert np.array_equal(clr.cpu().numpy().view(np.uint32), want["clearance"].view(np.uint32)) and np.array_equal(infl.cpu().numpy().view(np.uint64), want["inflated"])
    assert cnt.cpu().tolist() == want["counts"]
    wh, wc = D.query(want["dist2"], origin, DIMS, spheres, VS)
    print("camera centres:", [(int(h["code"]), int(h["dist2"])) for h in wh], wc)
    assert hits.cpu().numpy().tobytes() == wh.tobytes() and qcnt.cpu().tolist() == wc
    assert wh["code"][-1] != D.OUTSIDE and wh["code"][-1] != D.REJECTED  # the volume is centred on the last camera
    h = vm.distance_host(origin, DIMS, max_dist=MAX_DIST, inflate_radius=RADIUS)
    assert np.array_equal(h["dist2"].reshape(-1), want["dist2"]) and np.array_equal(h["nearest"].reshape(-1), want["nearest"])
    assert np.array_equal(h["inflated"], want["inflated"]) and [h["counts"][k] for k in api.DISTANCE_COUNTS] == want["counts"]
    after = vm.download()
    assert all(np.array_equal(before[k], after[k]) for k in before)  # nothing of this changes the map
    assert res1 == res0 and tabs1 == tabs0 and tracked1 == tracked0
    vm.close()
