"""GPU: a pipeline's keyframe clouds fused into a voxel map, and the map seen by rays from a later keyframe's pose (include/svo.h,
"Voxel map sight lines").  Three process calls with keyframe clouds on: the first keyframes' clouds are inserted
under their pose7; for every later keyframe the occupancy volume is formed around its pose, then its coarse volume, and the map
is cast at that pose by both walks at a quarter of the pipeline's image size.  Every view equals the restatement
(tests/voxel_rays_ref.py) over the downloaded table, and is handed to the carve of a second map in the format it is in.  Frame
results, tracked set and clouds are byte-identical to a run that never casts."""
import numpy as np
import pytest

import voxel_locate_ref as L
import voxel_rays_ref as R
from test_pipeline import _seq
from test_rectify import _bits, _params
from test_voxel_align_pipeline import _pose
from test_voxel_map_pipeline import DEPTH, H, LOG2, MD, VS, W, _bytes

pytestmark = pytest.mark.gpu
DIMS = (256, 64, 256)
VW, VH = W // 4, H // 4


def test_the_map_is_cast_at_later_keyframes_and_the_view_carves_a_second_map(ctx):
    import torch
    import stereo_vo_amd as S
    from stereo_vo_amd import api
    n, call = 12, 4
    p, Lt, Rt = _seq(n, w=W, h=H, seed=0x5EED0A00)
    pp = _params(S, p, MD)
    prm = api.CloudParams(2, 0.0, (W // 2) * (H // 2))
    cam = api.CameraInfo(pp.cam.focal / 4.0, pp.cam.cx / 4.0, pp.cam.cy / 4.0, 0, 0, 0, 0, pp.cam.baseline)
    cam4 = (cam.focal, cam.cx, cam.cy, cam.baseline)
    bits = torch.empty(api.voxel_occupancy_bytes(DIMS) // 8, dtype=torch.int64, device="cuda")
    coarse = torch.empty(api.voxel_occupancy_coarse_bytes(DIMS) // 8, dtype=torch.int64, device="cuda")
    occ = torch.zeros(2, dtype=torch.int32, device="cuda")

    def run(vm, second):
        pl = S.Pipeline(ctx, pp)
        pl.set_keyframe_clouds(prm)
        res, tabs, log = [], [], []
        for b0 in range(0, n, call):
            res += pl.process_batch(Lt[b0:b0 + call], Rt[b0:b0 + call])
            tab = pl.keyframe_clouds()
            for t in tab if vm is not None else ():
                pose = _pose(b0 + t["frame"])
                if vm.stats()["n_inserted"] > 0:
                    m12 = api.pose7_to_cam_to_world(pose).reshape(12)
                    origin = R.origin_of((m12[3], m12[7], m12[11]), VS, DIMS)
                    d = {k: v.copy() for k, v in vm.download().items()}
                    vm.occupancy(bits.data_ptr(), origin, DIMS, counts_ptr=occ.data_ptr())
                    vm.occupancy_coarse(bits.data_ptr(), DIMS, coarse.data_ptr())
                    words = L.occupancy_np(d, origin, DIMS, 1)[0]
                    want = R.raycast(words, origin, DIMS, VW, VH, cam4, m12, 30.0, 1, VS)
                    for c in (None, coarse.data_ptr()):
                        disp = torch.full((VW * VH,), 0x5555, dtype=torch.int16, device="cuda")
                        cell = torch.full((VW * VH,), -1, dtype=torch.int32, device="cuda")
                        cnt = torch.full((7,), -1, dtype=torch.int64, device="cuda")
                        torch.cuda.synchronize()
                        vm.raycast(bits.data_ptr(), origin, DIMS, VW, VH, cam, pose7=pose, coarse_ptr=c, disp_ptr=disp.data_ptr(), cell_ptr=cell.data_ptr(),
                                   counts_ptr=cnt.data_ptr())
                        ctx.sync()
                        assert np.array_equal(bits.cpu().numpy().view(np.uint64), words)
                        assert np.array_equal(disp.cpu().numpy().reshape(VH, VW), want[0]) and np.array_equal(cell.cpu().numpy().view(np.uint32).reshape(VH, VW), want[1])
                        assert cnt.cpu().tolist() == want[2], (cnt.cpu().tolist(), want[2])
                    second.carve(disp.data_ptr(), VW, VH, cam, pose7=pose)  # the view is a keyframe map in everything but its origin
                    ctx.sync()
                    after = vm.download()
                    assert all(np.array_equal(d[k], after[k]) for k in d)  # casting changes nothing in the map
                    log.append(want[2])
                vm.insert(t["dev"], t["n_stored"], pose7=pose)
                second.insert(t["dev"], t["n_stored"], pose7=pose)
            tabs += _bytes(tab)
        ids, xy = pl.tracked()
        pl.close()
        return [_bits(r) for r in res], tabs, (ids.tobytes(), xy.tobytes()), log

    res0, tabs0, tracked0, _ = run(None, None)
    vm = S.VoxelMap(ctx, voxel_size=VS, capacity_log2=LOG2, max_depth=DEPTH)
    second = S.VoxelMap(ctx, voxel_size=VS, capacity_log2=LOG2, max_depth=DEPTH)
    res1, tabs1, tracked1, log = run(vm, second)
    assert res1 == res0 and tabs1 == tabs0 and tracked1 == tracked0
    print("ray view counts per keyframe (n_hit, n_left, n_range, n_outside, n_rejected, n_steps, n_pixels):", log)
    assert len(log) >= 1 and all(c[6] >= 200 for c in log), log  # the map is seen
    second.close()
    vm.close()
