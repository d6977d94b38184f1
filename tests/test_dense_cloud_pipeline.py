"""GPU: keyframe clouds of a pipeline and of a pipeline group (include/svo.h, svo_pipeline_set_keyframe_clouds and the group's
form; src/image_processor.cpp:173-207 per keyframe).  Turning clouds on changes no bit of the frame results; every keyframe's cloud
equals the stand-alone svo_stereo_cloud of that pair, which tests/test_dense_cloud.py pins to the oracle."""
import ctypes as C

import numpy as np
import pytest

from test_pipeline import _seq
from test_rectify import _bits, _params

pytestmark = pytest.mark.gpu

W, H, N, CALL, MD = 496, 160, 12, 4, 10.0


def _same(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _run(pl, L, R, call):
    res = []
    for b0 in range(0, len(L), call):
        res += pl.process_batch(L[b0:b0 + call], R[b0:b0 + call])
    return res


@pytest.fixture(scope="module")
def rig():
    """Own context (496 x 160, room for the 12 frames in one call), the synthetic stream, and the run WITHOUT clouds."""
    import stereo_vo_amd as S
    p, L, R = _seq(N, w=W, h=H, seed=0x5EED0A00)
    c = S.Context(W, H, max_batch=N, max_corners=600, max_candidates=1 << 17, max_features=600)
    pp = _params(S, p, MD)
    ref = S.Pipeline(c, pp)
    res = _run(ref, L, R, CALL)
    tracked = ref.tracked()
    ref.close()
    kf = [r.is_keyframe for r in res]
    assert kf[0] == 1 and sum(kf) >= 2, kf
    cam = S.CameraInfo(p.focal, p.cx, p.cy, 0, 0, 0, 0, p.baseline)
    yield dict(S=S, p=p, L=L, R=R, ctx=c, pp=pp, res=res, tracked=tracked, cam=cam)
    c.close()


def test_pipeline_clouds_change_nothing_and_equal_the_stand_alone_clouds(rig):
    S, c, L, R = rig["S"], rig["ctx"], rig["L"], rig["R"]
    from stereo_vo_amd import api
    pl = S.Pipeline(c, rig["pp"])
    pl.set_keyframe_clouds(True)
    res, n_clouds = [], 0
    for b0 in range(0, N, CALL):
        c.profile_select("stereo_dense_batch")
        r = pl.process_batch(L[b0:b0 + CALL], R[b0:b0 + CALL])
        dense_launches = c.profile_read()[1]
        c.profile_select(None)
        res += r
        tab = pl.keyframe_clouds()
        # (b) exactly the keyframes of this call, in order
        assert [t["frame"] for t in tab] == [i for i, x in enumerate(r) if x.is_keyframe]
        assert all(t["lane"] == 0 for t in tab)
        assert dense_launches == (1 if tab else 0)
        # (c) each cloud is the stand-alone cloud of that pair, identity pose
        for t in tab:
            want, n_total = c.stereo_cloud(L[b0 + t["frame"]], R[b0 + t["frame"]], rig["cam"])
            assert n_total >= 1000, n_total
            assert t["n_total"] == n_total and t["n_stored"] == len(want)
            assert _same(t["points"], want), (b0, t["frame"])
            n_clouds += 1
    # (a) the frame results and the tracked set are those of the run without clouds
    assert [_bits(x) for x in res] == [_bits(x) for x in rig["res"]]
    ids, xy = pl.tracked()
    assert np.array_equal(ids, rig["tracked"][0]) and np.array_equal(xy.view(np.uint32), rig["tracked"][1].view(np.uint32))
    assert n_clouds == sum(x.is_keyframe for x in res) >= 2
    # a step / bound / cap of the caller's: the same clouds thinned and cut
    pl.set_keyframe_clouds(api.CloudParams(4, 1.5, 500))
    pl.reset()
    r = pl.process_batch(L[:CALL], R[:CALL])
    tab = pl.keyframe_clouds()
    assert [t["frame"] for t in tab] == [i for i, x in enumerate(r) if x.is_keyframe] and tab
    for t in tab:
        want, n_total = c.stereo_cloud(L[t["frame"]], R[t["frame"]], rig["cam"], None, 4, 1.5, 500)
        assert n_total > 500 and t["n_total"] == n_total and t["n_stored"] == 500 and _same(t["points"], want)
    # (d) off again: no launch
    pl.set_keyframe_clouds(None)
    pl.reset()
    res = []
    launches = 0
    for what in ("stereo_dense_batch", "cloud"):
        pl.reset()
        c.profile_select(what)
        res = _run(pl, L, R, CALL)
        launches += c.profile_read()[1]
        c.profile_select(None)
    assert launches == 0
    assert [_bits(x) for x in res] == [_bits(x) for x in rig["res"]]
    with pytest.raises(S.SvoError):
        pl.keyframe_clouds()
    pl.close()


def test_more_keyframes_than_the_bound_is_a_loud_capacity_error(rig):
    S, c, L, R = rig["S"], rig["ctx"], rig["L"], rig["R"]
    from stereo_vo_amd import api
    pl = S.Pipeline(c, rig["pp"])
    pl.set_keyframe_clouds(True, 1)
    assert sum(x.is_keyframe for x in rig["res"]) >= 2
    # all 12 frames in one call: at least two keyframes against a bound of one
    out = (api.FrameResult * N)()
    rc = c.L.svo_pipeline_process_batch(pl.h, L.ctypes.data_as(C.c_void_p), R.ctypes.data_as(C.c_void_p), N, out)
    assert rc == -3
    msg = c.L.svo_last_error(c.h).decode()
    assert "max_keyframes_per_call is 1" in msg, msg
    # the frame results are complete: those of one 12-frame call without clouds
    ref = S.Pipeline(c, rig["pp"])
    want = ref.process_batch(L, R)
    ref.close()
    assert [_bits(x) for x in out] == [_bits(x) for x in want]
    assert pl.keyframe_clouds() == []
    # after a reset the pipeline works, one keyframe per call fits the bound
    pl.reset()
    r = pl.process_batch(L[:1], R[:1])
    tab = pl.keyframe_clouds()
    assert r[0].is_keyframe == 1 and len(tab) == 1
    want, n_total = c.stereo_cloud(L[0], R[0], rig["cam"])
    assert tab[0]["n_total"] == n_total and _same(tab[0]["points"], want)
    pl.close()


def test_group_clouds_per_lane_with_a_rectified_lane(ctx):
    """Session context (max_batch 4): 2 lanes x 2 frames per call, 3 calls, different seeds; lane 1 is rectified (k1, p1)."""
    import torch
    import stereo_vo_amd as S
    from stereo_vo_amd import api
    lanes, batch, calls = 2, 2, 3
    n = batch * calls
    seqs = [_seq(n, w=W, h=H, seed=0x5EED0A00 + 17 * i) for i in range(lanes)]
    p = seqs[0][0]
    pp = _params(S, p, MD)
    cam = S.CameraInfo(p.focal, p.cx, p.cy, 0, 0, 0, 0, p.baseline)
    eye = api.rectify_eye(p.focal, p.focal, p.cx, p.cy, k1=-0.03, p1=2e-4)
    Ls, Rs = np.stack([s[1] for s in seqs]), np.stack([s[2] for s in seqs])
    # what lane 1's stages read: the output of svo_rectify_remap
    Lu = [Ls[0], np.stack([ctx.rectify_remap(x, eye, cam) for x in Ls[1]])]
    Ru = [Rs[0], np.stack([ctx.rectify_remap(x, eye, cam) for x in Rs[1]])]
    assert (Lu[1] != Ls[1]).mean() > 0.05

    g = S.PipelineGroup(ctx, pp, lanes)
    g.set_rectification(1, eye, eye)

    def run(entry, check):
        out = [[] for _ in range(lanes)]
        seen = 0
        for b0 in range(0, n, batch):
            if entry == "dev":
                dl, dr = torch.from_numpy(Ls[:, b0:b0 + batch].copy()).cuda(), torch.from_numpy(Rs[:, b0:b0 + batch].copy()).cuda()
                res = g.process_batch_dev(dl.data_ptr(), dr.data_ptr(), batch * W * H, batch)
                torch.cuda.synchronize()
            elif entry == "uploaded":
                sl, sr = g.staging(0)
                sl[:, :batch], sr[:, :batch] = Ls[:, b0:b0 + batch], Rs[:, b0:b0 + batch]
                g.upload(0, batch)
                res = g.process_uploaded(0, batch)
            else:
                res = g.process_batch(Ls[:, b0:b0 + batch], Rs[:, b0:b0 + batch])
            for l in range(lanes):
                out[l] += [_bits(r) for r in res[l]]
            if check is not None:
                tab = g.keyframe_clouds()
                assert [(t["lane"], t["frame"]) for t in tab] == [(l, i) for l in check for i in range(batch) if res[l][i].is_keyframe]
                for t in tab:
                    l, f = t["lane"], b0 + t["frame"]
                    want, n_total = ctx.stereo_cloud(Lu[l][f], Ru[l][f], cam)
                    assert n_total >= 1000 and t["n_total"] == n_total and _same(t["points"], want), (entry, l, f)
                seen += len(tab)
        return out, seen

    plain, _ = run("dev", None)  # the same group without clouds
    assert sum(b[4] for l in range(lanes) for b in plain[l]) >= lanes  # every lane's first frame at least
    for entry in ("dev", "uploaded", "host"):
        g.reset()
        g.set_keyframe_clouds(-1, True)
        got, seen = run(entry, range(lanes))
        assert got == plain, entry
        assert seen == sum(b[4] for l in range(lanes) for b in plain[l])
    # clouds on lane 0 only: no entry of lane 1
    g.reset()
    g.set_keyframe_clouds(-1, None)
    g.set_keyframe_clouds(0, True)
    got, seen = run("dev", [0])
    assert got == plain and seen == sum(b[4] for b in plain[0]) >= 1
    # off everywhere: no launch
    g.set_keyframe_clouds(-1, None)
    g.reset()
    ctx.profile_select("stereo_dense_batch")
    got, _ = run("dev", None)
    launches = ctx.profile_read()[1]
    ctx.profile_select(None)
    assert got == plain and launches == 0
    g.close()
