"""GPU: a voxel map filled from the keyframe clouds of a pipeline, and its grid (include/svo.h, "Voxel map grid").
After every one of three process calls the call's clouds are inserted under their frame's pose7 and the grid is built on the
pipeline's own stream.  Every grid equals the restatement (tests/voxel_grid_ref.py) applied to svo_voxel_map_download's table at that
moment; building grids changes no bit of the frame results, the tracked set or the clouds."""
import numpy as np
import pytest

import voxel_grid_ref as G
import voxel_ref as V
from test_pipeline import _seq
from test_rectify import _bits, _params
from test_voxel_grid import _eq, _grid
from test_voxel_map import _stored
from test_voxel_map_pipeline import DEPTH, H, LOG2, MD, VS, W, _bytes, _pose

pytestmark = pytest.mark.gpu

# the camera convention; 0.6 m cells (3 voxels of 0.2 m), 50 x 50 of them from 6 m behind the first camera, centred on its axis: wider
# than the clouds' depth bound and the poses' motion together
PARAMS = G.Params(1, -1, -6.0, -15.0, 3, 50, 50, -10.0, 10.0, 0.3, 1)


def test_pipeline_keyframe_clouds_into_a_grid(ctx):
    import stereo_vo_amd as S
    from stereo_vo_amd import api
    n, call = 12, 4
    p, L, R = _seq(n, w=W, h=H, seed=0x5EED0A00)
    pp = _params(S, p, MD)
    prm = api.CloudParams(2, 0.0, (W // 2) * (H // 2))

    def run(vm):
        pl = S.Pipeline(ctx, pp)
        pl.set_keyframe_clouds(prm)
        res, tabs, grids = [], [], []
        for b0 in range(0, n, call):
            res += pl.process_batch(L[b0:b0 + call], R[b0:b0 + call])
            tab = pl.keyframe_clouds()
            tabs += _bytes(tab)
            if vm is not None:
                vm.insert_keyframe_clouds(tab, [_pose(0, b0 + t["frame"]) for t in tab])  # before the next call replaces the clouds
                got = _grid(vm, PARAMS)
                grids.append((got, V.Table(*_stored(vm), 0, 0)))
        ids, xy = pl.tracked()
        pl.close()
        return [_bits(r) for r in res], tabs, (ids.tobytes(), xy.tobytes()), grids

    res0, tabs0, tracked0, _ = run(None)
    assert len(tabs0) >= 3
    vm = S.VoxelMap(ctx, voxel_size=VS, capacity_log2=LOG2, max_depth=DEPTH)
    res1, tabs1, tracked1, grids = run(vm)
    assert res1 == res0 and tabs1 == tabs0 and tracked1 == tracked0
    assert len(grids) == 3  # one per process call
    seen = []
    for got, down in grids:
        assert V.longest_run(V.occupied(down.keys, LOG2)) < V.MAX_PROBES
        w = G.grid_np(down, PARAMS, VS)
        assert G.same(w, G.grid_py(down, PARAMS, VS))
        print("grid counts (n_qualifying, n_in_band, n_binned, n_cells, n_obstacle):", w.counts)
        assert w.counts[2] >= 100 and w.counts[3] >= 10  # voxels are binned
        _eq(got, w)
        seen.append(w.counts)
    assert len(set(seen)) >= 2  # the map grew between the grids
    vm.close()
