"""GPU: a pipeline's keyframe clouds located in a voxel map from a pose several voxels away (include/svo.h, "Voxel map locate";
INTEGRATION 4a).  Three process calls with keyframe clouds on: the first keyframe's cloud is inserted under its pose7; every later
keyframe's cloud is located from its pose7 moved by (3.3, -1.2, 2.6) voxels and turned by 0.05 rad about the world's y, from the
table's device pointer, and then inserted under the result.  Everything equals the restatement (tests/voxel_locate_ref.py) over the
host copies of the same clouds and the downloaded table; frame results, tracked set and clouds are byte-identical to a run that
never locates."""
import ctypes as C

import numpy as np
import pytest

import voxel_align_ref as A
import voxel_locate_ref as L
import voxel_ref as V
from test_pipeline import _seq
from test_rectify import _bits, _params
from test_voxel_align_pipeline import _f64bits, _pose
from test_voxel_locate import restated
from test_voxel_map_pipeline import DEPTH, H, LOG2, MD, VS, W, _bytes

pytestmark = pytest.mark.gpu


def test_keyframe_clouds_located_before_they_are_inserted(ctx):
    import torch
    import stereo_vo_amd as S
    from stereo_vo_amd import api
    n, call = 12, 4
    p, Lt, R = _seq(n, w=W, h=H, seed=0x5EED0A00)
    pp = _params(S, p, MD)
    prm = api.CloudParams(2, 0.0, (W // 2) * (H // 2))
    lp = L.default_params(n_turn=2, turn_step=0.05, box=(5, 3, 5), dims=(256, 128, 256))
    ap = A.default_params(VS, max_iters=4)
    q = api._params(lambda: api.voxel_locate_default_params(VS), None, n_turn=lp.n_turn, turn_step=lp.turn_step)
    q.box, q.dims = (C.c_int * 3)(*lp.box), (C.c_int * 3)(*lp.dims)
    ws = torch.empty(api.voxel_locate_workspace_bytes(q) + 256, dtype=torch.uint8, device="cuda")
    wptr = (ws.data_ptr() + 255) & ~255

    def run(vm):
        pl = S.Pipeline(ctx, pp)
        pl.set_keyframe_clouds(prm)
        res, tabs, log = [], [], []
        for b0 in range(0, n, call):
            res += pl.process_batch(Lt[b0:b0 + call], R[b0:b0 + call])
            tab = pl.keyframe_clouds()
            for t in tab if vm is not None else ():
                pose = _pose(b0 + t["frame"])
                if vm.stats()["n_inserted"] == 0:
                    vm.insert(t["dev"], t["n_stored"], pose7=pose)
                    continue
                d = {k: v.copy() for k, v in vm.download().items()}
                pts = t["points"].view(V.POINT)
                start = L.start_pose(pose, [3.3 * VS, -1.2 * VS, 2.6 * VS], 0.05)
                got_out, got = vm.locate(t["dev"], t["n_stored"], np.array(start), params=q, align_params=api._params(lambda: api.voxel_align_default_params(VS), None, **ap._asdict()),
                                         workspace_ptr=wptr)
                out, want, _ = restated(d, None, pts, start, lp, ap, VS, DEPTH)
                assert _f64bits(got_out) == _f64bits(out) and _f64bits(got["coarse_pose7"]) == _f64bits(want["coarse_pose7"]), (got, want)
                assert _f64bits(got["align"]["xi"]) == _f64bits(want["align"]["xi"])
                plain = lambda r: ({k: v for k, v in r.items() if k not in ("coarse_pose7", "align")}, {k: v for k, v in r["align"].items() if k != "xi"})
                assert plain(got) == plain(want), (got, want)
                log.append((want["status"], want["hits"], A.pose_errors(start, pose)[0], A.pose_errors(out, pose)[0]))
                after = vm.download()
                assert all(np.array_equal(d[k], after[k]) for k in d)  # locating changes nothing in the map
                vm.insert(t["dev"], t["n_stored"], pose7=got_out)
            tabs += _bytes(tab)
        ids, xy = pl.tracked()
        pl.close()
        return [_bits(r) for r in res], tabs, (ids.tobytes(), xy.tobytes()), log

    res0, tabs0, tracked0, _ = run(None)
    vm = S.VoxelMap(ctx, voxel_size=VS, capacity_log2=LOG2, max_depth=DEPTH)
    res1, tabs1, tracked1, log = run(vm)
    assert res1 == res0 and tabs1 == tabs0 and tracked1 == tracked0
    print(log)
    assert len(log) >= 1 and all(t0 > 3 * VS for _, _, t0, _ in log) and any(status == "FOUND" and hits > 64 for status, hits, _, _ in log), log
    vm.close()
