"""GPU: keyframe maps of a pipeline and of a pipeline group used to carve voxel maps (include/svo.h, "Free-space carving";
INTEGRATION 4a).  Every keyframe's map, reached through keyframe_disparity on the device, first carves what the earlier keyframes put
into the map, under the keyframe's pose7; then its cloud is inserted.  The result equals the restatement (tests/voxel_carve_ref.py,
tests/voxel_ref.py) over the host copies of the same maps and clouds; carving changes no bit of the frame results, the tracked set
or the clouds.

keyframe_disparity and copy_keyframe_disparity share their lookup, so the map is tied to its cloud by a route that uses neither: the
cloud rule (test_dense_cloud._expected_cloud: the step rule and the oracle's triangulation) over the host map and the left image of
entry i's frame reproduces entry i's cloud, record for record.  A wrong entry, another lane's map or an unfiltered map would not.
Both tests run with the filters off and with the left-right check and the speckle filter on, where the maps must also differ from
the unfiltered ones."""
import numpy as np
import pytest

import voxel_carve_ref as R
import voxel_ref as V
from test_dense_cloud import _expected_cloud, _same
from test_pipeline import _seq
from test_rectify import _bits, _params
from test_voxel_map_pipeline import DEPTH, H, LOG2, MD, VS, W, _bytes, _pose

pytestmark = pytest.mark.gpu

RADIUS, MARGIN16, KEEP = 1, 8, 0
STEP = 2  # of the keyframe clouds


def _filters(pipe, on):
    if on:
        pipe.set_keyframe_lr_check(16)
        pipe.set_keyframe_speckle_filter(100, 32)


def _assert_map_forms_cloud(disp, left, cam, entry, what):
    """Entry's cloud is the cloud of THIS map and THIS frame's left image (max_points is the whole grid: nothing is cut)."""
    want = _expected_cloud(left, disp, cam, STEP, 0.0, None)
    assert entry["n_total"] == entry["n_stored"] == len(want) >= 1000, what
    assert _same(want, entry["points"]), what


def _carve_then_insert(vm, src, tab, poses, cam, counts):
    """src: the Pipeline or PipelineGroup the table came from; tab: (index in the table, entry) pairs."""
    import torch
    for (i, e), q in zip(tab, poses):
        cnt = torch.full((3,), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        vm.carve(src.keyframe_disparity(i), W, H, cam, pose7=q, radius=RADIUS, margin16=MARGIN16, keep_count=KEEP, counts_ptr=cnt.data_ptr())
        vm.insert(e["dev"], e["n_stored"], pose7=q)
        vm.ctx.sync()
        counts.append(tuple(cnt.cpu().tolist()))


def _want(entries, cam):
    """The restatement over (host map, host points, pose7) triples: (Table, the counts of every carve)."""
    from stereo_vo_amd import api
    cam4 = (cam.focal, cam.cx, cam.cy, cam.baseline)
    want, counts = R.empty_table(), []
    for disp, pts, pose in entries:
        want, c = R.carve_np(want, disp, cam4, api.pose7_to_world_to_cam(pose), VS, RADIUS, MARGIN16, KEEP)
        counts.append(c)
        want = V.merge(want, V.insert_np(pts.view(V.POINT), api.pose7_to_cam_to_world(pose), VS, DEPTH))
    return want, counts


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


@pytest.mark.parametrize("filters", (False, True))
def test_pipeline_keyframe_maps_carve_a_map(ctx, filters):
    import stereo_vo_amd as S
    from stereo_vo_amd import api
    n, call = 12, 4
    p, L, Rr = _seq(n, w=W, h=H, seed=0x5EED0A00)
    pp = _params(S, p, MD)
    prm = api.CloudParams(STEP, 0.0, (W // STEP) * (H // STEP))

    def run(vm, filters=filters):
        pl = S.Pipeline(ctx, pp)
        pl.set_keyframe_clouds(prm)
        _filters(pl, filters)
        res, tabs, entries, counts, per_call = [], [], [], [], []
        for b0 in range(0, n, call):
            res += pl.process_batch(L[b0:b0 + call], Rr[b0:b0 + call])
            tab = pl.keyframe_clouds()
            per_call.append(len(tab))
            poses = [_pose(0, b0 + t["frame"]) for t in tab]
            if vm is not None:
                _carve_then_insert(vm, pl, list(enumerate(tab)), poses, pp.cam, counts)  # before the next call replaces the maps
            tabs += _bytes(tab)
            for (i, t), q in zip(enumerate(tab), poses):
                disp = pl.copy_keyframe_disparity(i)
                _assert_map_forms_cloud(disp, L[b0 + t["frame"]], pp.cam, t, (b0, i))
                entries.append((disp, t["points"], q))
        ids, xy = pl.tracked()
        pl.close()
        assert max(per_call) >= 2  # an entry other than the first of its call
        return [_bits(r) for r in res], tabs, entries, (ids.tobytes(), xy.tobytes()), counts

    res0, tabs0, entries, tracked0, _ = run(None)
    if filters:  # the filters took something away: these are not the maps of the dense launch
        plain = run(None, False)[2]
        assert len(plain) == len(entries) and all((a[0] != b[0]).sum() >= 100 and len(a[1]) < len(b[1]) for a, b in zip(entries, plain))
    assert len(entries) >= 2 and all(e[0].shape == (H, W) and (e[0] > 0).sum() >= 1000 for e in entries)
    vm = S.VoxelMap(ctx, voxel_size=VS, capacity_log2=LOG2, max_depth=DEPTH)
    res1, tabs1, entries1, tracked1, counts = run(vm)
    assert res1 == res0 and tabs1 == tabs0 and tracked1 == tracked0
    assert all(np.array_equal(a[0], b[0]) for a, b in zip(entries, entries1))
    want, want_counts = _want(entries, pp.cam)
    print("carve counts per keyframe (n_live, n_tested, n_carved):", want_counts)
    assert want_counts[0] == (0, 0, 0) and sum(c[2] for c in want_counts) >= 100  # the first keyframe meets an empty map; later ones carve
    assert V.longest_run(V.occupied(want.keys, LOG2)) < V.MAX_PROBES
    assert counts == want_counts
    _assert_map(vm, want, sum(len(e[1]) for e in entries))
    vm.close()


@pytest.mark.parametrize("filters", (False, True))
def test_group_keyframe_maps_carve_one_map_per_lane(ctx, filters):
    import stereo_vo_amd as S
    from stereo_vo_amd import api
    lanes, batch, calls = 2, 2, 3
    n = batch * calls
    seqs = [_seq(n, w=W, h=H, seed=0x5EED0A00 + 17 * i) for i in range(lanes)]
    pp = _params(S, seqs[0][0], MD)
    Ls, Rs = np.stack([s[1] for s in seqs]), np.stack([s[2] for s in seqs])
    prm = api.CloudParams(STEP, 0.0, (W // STEP) * (H // STEP))

    def run(maps, filters=filters):
        g = S.PipelineGroup(ctx, pp, lanes)
        g.set_keyframe_clouds(-1, prm)
        _filters(g, filters)
        res, tabs, entries, counts = [[] for _ in range(lanes)], [], [[] for _ in range(lanes)], [[] for _ in range(lanes)]
        later = 0  # entries that are not the first of their call's table
        for b0 in range(0, n, batch):
            r = g.process_batch(Ls[:, b0:b0 + batch], Rs[:, b0:b0 + batch])
            tab = g.keyframe_clouds()
            for l in range(lanes):
                res[l] += [_bits(x) for x in r[l]]
                mine = [(i, t) for i, t in enumerate(tab) if t["lane"] == l]
                poses = [_pose(l, b0 + t["frame"]) for _, t in mine]
                if maps is not None:
                    _carve_then_insert(maps[l], g, mine, poses, pp.cam, counts[l])
                for (i, t), q in zip(mine, poses):
                    disp = g.copy_keyframe_disparity(i)
                    _assert_map_forms_cloud(disp, Ls[l, b0 + t["frame"]], pp.cam, t, (b0, i, l))
                    entries[l].append((disp, t["points"], q))
                    later += i != 0
            tabs += _bytes(tab)
        tracked = [tuple(a.tobytes() for a in g.get_tracked(l)) for l in range(lanes)]
        g.close()
        assert later >= 1
        return res, tabs, entries, counts, tracked

    res0, tabs0, entries, _, tracked0 = run(None)
    assert all(len(e) >= 1 for e in entries) and sum(len(e) for e in entries) >= 3
    if filters:
        plain = run(None, False)[2]
        for e, pe in zip(entries, plain):
            assert len(pe) == len(e) and all((a[0] != b[0]).sum() >= 100 and len(a[1]) < len(b[1]) for a, b in zip(e, pe))
    maps = [S.VoxelMap(ctx, voxel_size=VS, capacity_log2=LOG2, max_depth=DEPTH) for _ in range(lanes)]
    res1, tabs1, _, counts, tracked1 = run(maps)
    assert res1 == res0 and tabs1 == tabs0 and tracked1 == tracked0 and all(len(t[0]) > 0 for t in tracked0)
    for vm, e, c in zip(maps, entries, counts):
        want, want_counts = _want(e, pp.cam)
        print("carve counts per keyframe (n_live, n_tested, n_carved):", want_counts)
        assert V.longest_run(V.occupied(want.keys, LOG2)) < V.MAX_PROBES
        assert want_counts[0] == (0, 0, 0) and sum(x[2] for x in want_counts) >= 100
        assert c == want_counts
        _assert_map(vm, want, sum(len(x[1]) for x in e))
        vm.close()
