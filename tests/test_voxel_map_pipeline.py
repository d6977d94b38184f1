"""GPU: keyframe clouds of a pipeline and of a pipeline group fused into voxel maps (include/svo.h, "voxel map").
VoxelMap.insert_keyframe_clouds over several process calls, from the tables' device pointers, equals the restatement
(tests/voxel_ref.py, which tests/test_voxel_map.py shows to agree with itself by two routes) over the host copies of the same clouds;
inserting changes no bit of the frame results or of the clouds."""
import numpy as np
import pytest

import voxel_ref as V
from test_pipeline import _seq
from test_rectify import _bits, _params

pytestmark = pytest.mark.gpu

W, H, MD = 496, 160, 10.0
VS, LOG2, DEPTH = 0.2, 17, 15.0


def _pose(lane, frame):
    """A pose7 per keyframe, a non-unit quaternion: what a caller would take from results[i].pose7 / svo_ba_get_pose."""
    return np.array([1.0, 0.01 * frame, -0.02 * frame + 0.05 * lane, 0.003 * frame, 0.1 * frame, 0.3 * lane, 0.05 * frame])


def _bytes(tab):
    return [(t["frame"], t["lane"], t["n_total"], t["n_stored"], t["points"].tobytes()) for t in tab]


def _want(entries):
    """The restatement over (host points, pose7) pairs."""
    from stereo_vo_amd import api
    want = None
    for pts, pose in entries:
        t = V.insert_np(pts.view(V.POINT), api.pose7_to_cam_to_world(pose), VS, DEPTH)
        want = t if want is None else V.merge(want, t)
    return want


def _assert_map(vm, want, n_given):
    d = vm.download()
    occ = d["keys"] != np.uint64(V.EMPTY)
    o = np.argsort(d["keys"][occ])
    for name in ("keys", "ci", "sx", "sy", "sz"):
        assert np.array_equal(d[name][occ][o], getattr(want, name)), name
    assert vm.stats() == {"n_voxels": len(want.keys), "n_inserted": want.n_inserted, "n_rejected": want.n_rejected, "n_dropped": 0}
    assert want.n_inserted + want.n_rejected == n_given
    pts, n_total = vm.extract(2)
    assert n_total == len(pts) and np.array_equal(V.sort_records(pts), V.extract(want, VS, 2))


def test_pipeline_keyframe_clouds_into_a_map(ctx):
    import stereo_vo_amd as S
    from stereo_vo_amd import api
    n, call = 12, 4
    p, L, R = _seq(n, w=W, h=H, seed=0x5EED0A00)
    pp = _params(S, p, MD)
    prm = api.CloudParams(2, 0.0, (W // 2) * (H // 2))

    def run(vm):
        pl = S.Pipeline(ctx, pp)
        pl.set_keyframe_clouds(prm)
        res, tabs, entries = [], [], []
        for b0 in range(0, n, call):
            res += pl.process_batch(L[b0:b0 + call], R[b0:b0 + call])
            tab = pl.keyframe_clouds()
            poses = [_pose(0, b0 + t["frame"]) for t in tab]
            if vm is not None:
                vm.insert_keyframe_clouds(tab, poses)  # before the next call replaces the clouds
            tabs += _bytes(tab)
            entries += [(t["points"], q) for t, q in zip(tab, poses)]
        ids, xy = pl.tracked()
        pl.close()
        return [_bits(r) for r in res], tabs, entries, (ids.tobytes(), xy.tobytes())

    # with no map anywhere: the existing wrappers' outputs
    res0, tabs0, entries, tracked0 = run(None)
    assert len(entries) >= 2 and sum(len(e[0]) for e in entries) >= 2000
    vm = S.VoxelMap(ctx, voxel_size=VS, capacity_log2=LOG2, max_depth=DEPTH)
    res1, tabs1, _, tracked1 = run(vm)
    assert res1 == res0 and tabs1 == tabs0 and tracked1 == tracked0
    want = _want(entries)
    assert want.n_inserted >= 1000 and want.n_rejected >= 1 and len(want.keys) >= 100  # the depth bound cuts something
    assert V.longest_run(V.occupied(want.keys, LOG2)) < V.MAX_PROBES
    _assert_map(vm, want, sum(len(e[0]) for e in entries))
    with pytest.raises(ValueError):
        vm.insert_keyframe_clouds([{"dev": 0, "n_stored": 0}], [])
    vm.close()


def test_group_keyframe_clouds_into_one_map_per_lane(ctx):
    import stereo_vo_amd as S
    from stereo_vo_amd import api
    lanes, batch, calls = 2, 2, 3
    n = batch * calls
    seqs = [_seq(n, w=W, h=H, seed=0x5EED0A00 + 17 * i) for i in range(lanes)]
    pp = _params(S, seqs[0][0], MD)
    Ls, Rs = np.stack([s[1] for s in seqs]), np.stack([s[2] for s in seqs])
    prm = api.CloudParams(2, 0.0, (W // 2) * (H // 2))

    def run(maps):
        g = S.PipelineGroup(ctx, pp, lanes)
        g.set_keyframe_clouds(-1, prm)
        res, tabs, entries = [[] for _ in range(lanes)], [], [[] for _ in range(lanes)]
        for b0 in range(0, n, batch):
            r = g.process_batch(Ls[:, b0:b0 + batch], Rs[:, b0:b0 + batch])
            tab = g.keyframe_clouds()
            for l in range(lanes):
                res[l] += [_bits(x) for x in r[l]]
                mine = [t for t in tab if t["lane"] == l]
                poses = [_pose(l, b0 + t["frame"]) for t in mine]
                if maps is not None:
                    maps[l].insert_keyframe_clouds(mine, poses)
                entries[l] += [(t["points"], q) for t, q in zip(mine, poses)]
            tabs += _bytes(tab)
        g.close()
        return res, tabs, entries

    res0, tabs0, entries = run(None)
    assert all(len(e) >= 1 for e in entries) and sum(len(e) for e in entries) >= 3
    maps = [S.VoxelMap(ctx, voxel_size=VS, capacity_log2=LOG2, max_depth=DEPTH) for _ in range(lanes)]
    res1, tabs1, _ = run(maps)
    assert res1 == res0 and tabs1 == tabs0
    wants = [_want(e) for e in entries]
    assert not np.array_equal(wants[0].keys, wants[1].keys)
    for vm, want, e in zip(maps, wants, entries):
        assert V.longest_run(V.occupied(want.keys, LOG2)) < V.MAX_PROBES
        _assert_map(vm, want, sum(len(x[0]) for x in e))
        vm.close()
