"""GPU: voxel maps filled from the keyframe clouds of a pipeline and of a pipeline group, rendered at a keyframe's pose (include/svo.h,
"Voxel map render").  After every process call the call's clouds are inserted under their pose7 and the map is
rendered at the pose of the last keyframe so far, on the pipeline's own stream between two process calls.  Every render equals the
restatement (tests/voxel_render_ref.py over tests/voxel_ref.py) on the host copies of the same clouds; rendering changes no bit of the
frame results, the tracked set or the clouds."""
import numpy as np
import pytest

import voxel_ref as V
import voxel_render_ref as RR
from test_pipeline import _seq
from test_rectify import _bits, _params
from test_voxel_map_pipeline import DEPTH, H, LOG2, MD, VS, W, _bytes, _pose

pytestmark = pytest.mark.gpu


class _Target:
    """Device buffers of one render, kept until the stream has passed it."""

    def __init__(self):
        import torch
        n = W * H
        self.ws = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        self.disp = torch.full((n,), 0x5555, dtype=torch.int16, device="cuda")
        self.inten = torch.full((n,), 0xAA, dtype=torch.uint8, device="cuda")
        self.cnt = torch.full((4,), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()

    def render(self, vm, cam, pose7):
        vm.render(W, H, cam, pose7=pose7, workspace_ptr=self.ws.data_ptr(), disp_ptr=self.disp.data_ptr(), intensity_ptr=self.inten.data_ptr(),
                  counts_ptr=self.cnt.data_ptr())

    def read(self, vm):
        vm.ctx.sync()
        return self.disp.cpu().numpy().reshape(H, W), self.inten.cpu().numpy().reshape(H, W), tuple(self.cnt.cpu().tolist())


def _want(entries, upto, cam, pose7):
    """The restatement's render of the map of entries[:upto] ((host points, pose7) pairs) at pose7."""
    from stereo_vo_amd import api
    t = None
    for pts, q in entries[:upto]:
        one = V.insert_np(pts.view(V.POINT), api.pose7_to_cam_to_world(q), VS, DEPTH)
        t = one if t is None else V.merge(t, one)
    assert V.longest_run(V.occupied(t.keys, LOG2)) < V.MAX_PROBES
    return RR.render_np(t, W, H, (cam.focal, cam.cx, cam.cy, cam.baseline), api.pose7_to_world_to_cam(pose7), VS)


def _assert_renders(got, entries, cam):
    assert len(got) == 3  # one per process call
    seen = []
    for upto, pose, (disp, inten, counts) in got:
        w = _want(entries, upto, cam, pose)
        print("render counts (n_qualifying, n_drawn, n_splat, n_pixels):", w[2])
        assert w[2][1] >= 100 and w[2][3] >= 1000  # voxels are seen
        assert np.array_equal(disp, w[0]) and np.array_equal(inten, w[1]) and counts == w[2], upto
        seen.append(w[2])
    assert len(set(seen)) >= 2  # the map grew and the pose moved between the renders


def test_pipeline_keyframe_clouds_rendered_at_the_last_keyframe(ctx):
    import stereo_vo_amd as S
    from stereo_vo_amd import api
    n, call = 12, 4
    p, L, R = _seq(n, w=W, h=H, seed=0x5EED0A00)
    pp = _params(S, p, MD)
    prm = api.CloudParams(2, 0.0, (W // 2) * (H // 2))

    def run(vm):
        pl = S.Pipeline(ctx, pp)
        pl.set_keyframe_clouds(prm)
        res, tabs, entries, renders = [], [], [], []
        targets = [_Target() for _ in range(n // call)] if vm is not None else []  # up front: no synchronisation between the calls
        for b0 in range(0, n, call):
            res += pl.process_batch(L[b0:b0 + call], R[b0:b0 + call])
            tab = pl.keyframe_clouds()
            poses = [_pose(0, b0 + t["frame"]) for t in tab]
            tabs += _bytes(tab)
            entries += [(t["points"], q) for t, q in zip(tab, poses)]
            if vm is not None:
                vm.insert_keyframe_clouds(tab, poses)  # before the next call replaces the clouds
                target = targets.pop()
                target.render(vm, pp.cam, entries[-1][1])
                renders.append((len(entries), entries[-1][1], target))
        renders = [(upto, q, t.read(vm)) for upto, q, t in renders]  # read after the last call: nothing waited in between
        ids, xy = pl.tracked()
        pl.close()
        return [_bits(r) for r in res], tabs, entries, (ids.tobytes(), xy.tobytes()), renders

    res0, tabs0, entries, tracked0, _ = run(None)
    assert len(entries) >= 3
    vm = S.VoxelMap(ctx, voxel_size=VS, capacity_log2=LOG2, max_depth=DEPTH)
    res1, tabs1, _, tracked1, renders = run(vm)
    assert res1 == res0 and tabs1 == tabs0 and tracked1 == tracked0
    _assert_renders(renders, entries, pp.cam)
    vm.close()


def test_group_keyframe_clouds_rendered_per_lane(ctx):
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
        res, tabs, entries, renders = [[] for _ in range(lanes)], [], [[] for _ in range(lanes)], [[] for _ in range(lanes)]
        targets = [_Target() for _ in range(lanes * calls)] if maps is not None else []
        for b0 in range(0, n, batch):
            r = g.process_batch(Ls[:, b0:b0 + batch], Rs[:, b0:b0 + batch])
            tab = g.keyframe_clouds()
            for l in range(lanes):
                res[l] += [_bits(x) for x in r[l]]
                mine = [t for t in tab if t["lane"] == l]
                poses = [_pose(l, b0 + t["frame"]) for t in mine]
                entries[l] += [(t["points"], q) for t, q in zip(mine, poses)]
                if maps is not None:
                    maps[l].insert_keyframe_clouds(mine, poses)
                    assert entries[l]  # every lane has a keyframe in its first call
                    target = targets.pop()
                    target.render(maps[l], pp.cam, entries[l][-1][1])
                    renders[l].append((len(entries[l]), entries[l][-1][1], target))
            tabs += _bytes(tab)
        if maps is not None:
            renders = [[(upto, q, t.read(maps[l])) for upto, q, t in renders[l]] for l in range(lanes)]
        tracked = [tuple(a.tobytes() for a in g.get_tracked(l)) for l in range(lanes)]
        g.close()
        return res, tabs, entries, renders, tracked

    res0, tabs0, entries, _, tracked0 = run(None)
    assert all(len(e) >= 1 for e in entries) and sum(len(e) for e in entries) >= 3
    maps = [S.VoxelMap(ctx, voxel_size=VS, capacity_log2=LOG2, max_depth=DEPTH) for _ in range(lanes)]
    res1, tabs1, _, renders, tracked1 = run(maps)
    assert res1 == res0 and tabs1 == tabs0 and tracked1 == tracked0 and all(len(t[0]) > 0 for t in tracked0)
    for l, vm in enumerate(maps):
        assert len(renders[l]) == calls
        for upto, pose, (disp, inten, counts) in renders[l]:
            w = _want(entries[l], upto, pp.cam, pose)
            print("lane", l, "render counts (n_qualifying, n_drawn, n_splat, n_pixels):", w[2])
            assert w[2][1] >= 100 and w[2][3] >= 1000
            assert np.array_equal(disp, w[0]) and np.array_equal(inten, w[1]) and counts == w[2], (l, upto)
        vm.close()
    assert not np.array_equal(renders[0][-1][2][0], renders[1][-1][2][0])  # each lane sees its own map
