"""GPU: semi-global matching for the keyframe maps of a pipeline and of a pipeline group (include/svo.h,
svo_pipeline_set_keyframe_sgm and the group's form), on the stream tests/test_lr_check_pipeline.py uses.  Every keyframe's cloud
equals the triangulation of the restatement's map (tests/sgm_ref.py at (48, 21), then lr_check_ref.check_arrays fed by its cost
form and speckle_ref.filter_propagate where those switches are on), bit for bit; the frame results and the tracked set are those
of a run with nothing on; p1 = p2 = 0 gives the clouds of block matching; off again restores the plain launch sequence.

Points per keyframe of the pipeline's stream (frames 0, 4, 7, 10), semi-global matching with the defaults against block matching:
52,544 / 44,112, 54,987 / 47,715, 57,165 / 51,308, 56,777 / 52,805; with the check and the speckle filter on both sides 52,066 /
42,997, 54,052 / 46,343, 56,034 / 50,220, 55,070 / 52,147.  All twelve frames in one call hold more keyframes than one sub-batch: the loop runs twice."""
import numpy as np
import pytest

import lr_check_ref as LR
import sgm_ref as SG
import speckle_ref as SP
import stereo_bm_ref as BM
from test_dense_cloud import _expected_cloud, _same
from test_dense_cloud_pipeline import CALL, H, MD, N, W, _run
from test_pipeline import _seq
from test_rectify import _bits, _params

pytestmark = pytest.mark.gpu

MAX_DIFF = 16
SPECKLE = (100, 32)
_MAPS = {}


def _want(key, left, right, cam, sgm=True, checked=False, speckled=False):
    """The expected cloud of one rectified pair under the three switches; the maps of a pair are formed once per session (`key`)."""
    k = (key, sgm)
    if k not in _MAPS:
        _MAPS[k] = (SG.sgm(left, right, 48, 21) if sgm else (BM.stereo_bm(left, right, 48, 21), LR.min_sad(left, right, 48, 21)), {})
    (m, c), done = _MAPS[k]
    if (checked, speckled) not in done:
        use = LR.check_arrays(m, c, MAX_DIFF)[0] if checked else m
        if speckled:
            use = SP.filter_propagate(use, *SPECKLE)[0]
        done[checked, speckled] = _expected_cloud(left, use, cam, 1, 0.0, None)
    return done[checked, speckled]


def _launches(c, name, call):
    c.profile_select(name)
    out = call()
    n = c.profile_read()[1]
    c.profile_select(None)
    return out, n


@pytest.fixture(scope="module")
def rig():
    import stereo_vo_amd as S
    p, L, Rr = _seq(N, w=W, h=H, seed=0x5EED0A00)
    c = S.Context(W, H, max_batch=N, max_corners=600, max_candidates=1 << 17, max_features=600)
    pp = _params(S, p, MD)
    ref = S.Pipeline(c, pp)
    res = _run(ref, L, Rr, CALL)
    tracked = ref.tracked()
    ref.close()
    assert sum(r.is_keyframe for r in res) >= 2
    cam = S.CameraInfo(p.focal, p.cx, p.cy, 0, 0, 0, 0, p.baseline)
    yield dict(S=S, L=L, R=Rr, ctx=c, pp=pp, res=res, tracked=tracked, cam=cam)
    c.close()


@pytest.mark.parametrize("filtered", [False, True], ids=["sgm", "sgm_check_speckle"])
def test_pipeline_clouds_are_those_of_the_sgm_maps(rig, filtered):
    from stereo_vo_amd import api
    S, c, L, Rr, cam = rig["S"], rig["ctx"], rig["L"], rig["R"], rig["cam"]
    sub = api.SGM_KEYFRAME_SUB_BATCH
    pl = S.Pipeline(c, rig["pp"])
    with pytest.raises(S.SvoError, match="keyframe clouds are off"):
        pl.set_keyframe_sgm()
    pl.set_keyframe_clouds(True)
    for bad, word in (((9, 8), "p2"), ((-1, 8), "p1"), ((0, 32768), "SVO_SGM_MAX_P2")):
        with pytest.raises(S.SvoError, match=word):
            pl.set_keyframe_sgm(*bad)
    if filtered:
        pl.set_keyframe_lr_check(MAX_DIFF)
    pl.set_keyframe_sgm()
    if filtered:  # the switches are independent: either order
        pl.set_keyframe_speckle_filter(*SPECKLE)
    res, seen = [], 0
    for b0 in range(0, N, CALL):
        r, launches = _launches(c, "stereo_sgm", lambda: pl.process_batch(L[b0:b0 + CALL], Rr[b0:b0 + CALL]))
        res += r
        tab = pl.keyframe_clouds()
        assert [t["frame"] for t in tab] == [i for i, x in enumerate(r) if x.is_keyframe]
        assert launches == (len(tab) + sub - 1) // sub
        for t in tab:
            f = b0 + t["frame"]
            want = _want(("s0", f), L[f], Rr[f], cam, True, filtered, filtered)
            plain = _want(("s0", f), L[f], Rr[f], cam, False, filtered, filtered)
            print("keyframe", f, "points", len(want), "with block matching", len(plain))
            assert len(want) >= 1000 and not _same(want, plain)
            assert t["n_total"] == t["n_stored"] == len(want) and _same(t["points"], want), (b0, t["frame"])
            seen += 1
    assert seen == sum(x.is_keyframe for x in res) >= 2
    assert [_bits(x) for x in res] == [_bits(x) for x in rig["res"]]
    ids, xy = pl.tracked()
    assert np.array_equal(ids, rig["tracked"][0]) and np.array_equal(xy.view(np.uint32), rig["tracked"][1].view(np.uint32))
    # new cloud parameters keep the switch
    pl.set_keyframe_clouds(api.CloudParams(1, 0.0, W * H), 2)
    pl.reset()
    r = pl.process_batch(L[:1], Rr[:1])
    tab = pl.keyframe_clouds()
    assert r[0].is_keyframe == 1 and len(tab) == 1 and _same(tab[0]["points"], _want(("s0", 0), L[0], Rr[0], cam, True, filtered, filtered))
    # off again: the plain launch sequence and its clouds, the filters as they were
    pl.set_keyframe_sgm(on=False)
    pl.reset()
    r, launches = _launches(c, "stereo_sgm", lambda: pl.process_batch(L[:CALL], Rr[:CALL]))
    tab = pl.keyframe_clouds()
    assert launches == 0 and tab
    for t in tab:
        f = t["frame"]
        assert _same(t["points"], _want(("s0", f), L[f], Rr[f], cam, False, filtered, filtered))
    pl.reset()
    _, launches = _launches(c, "stereo_dense_batch", lambda: pl.process_batch(L[:CALL], Rr[:CALL]))
    assert launches == 1
    # clouds off frees the workspace with them: turning the switch on again needs the clouds first
    pl.set_keyframe_sgm()
    pl.set_keyframe_clouds(None)
    with pytest.raises(S.SvoError, match="keyframe clouds are off"):
        pl.set_keyframe_sgm()
    pl.close()


def test_more_keyframes_in_a_call_than_the_sub_batch_and_zero_penalties(rig):
    """All twelve frames in one call: the matching sequence runs once per sub-batch.  Then p1 = p2 = 0: the clouds without the switch."""
    from stereo_vo_amd import api
    S, c, L, Rr, cam = rig["S"], rig["ctx"], rig["L"], rig["R"], rig["cam"]
    sub = api.SGM_KEYFRAME_SUB_BATCH
    pl = S.Pipeline(c, rig["pp"])
    pl.set_keyframe_clouds(True)
    pl.process_batch(L, Rr)
    plain = pl.keyframe_clouds()
    assert len(plain) > sub, "the stream must put more keyframes into one call than SVO_SGM_KEYFRAME_SUB_BATCH"
    pl.set_keyframe_sgm()
    pl.reset()
    r, launches = _launches(c, "stereo_sgm", lambda: pl.process_batch(L, Rr))
    tab = pl.keyframe_clouds()
    assert [t["frame"] for t in tab] == [t["frame"] for t in plain] and launches == (len(tab) + sub - 1) // sub >= 2
    for t in tab:
        f = t["frame"]
        assert _same(t["points"], _want(("s0", f), L[f], Rr[f], cam)), f
    pl.set_keyframe_sgm(0, 0)
    pl.reset()
    _, launches = _launches(c, "stereo_sgm", lambda: pl.process_batch(L, Rr))
    tab = pl.keyframe_clouds()
    assert launches >= 2 and len(tab) == len(plain)
    for t, q in zip(tab, plain):
        assert t["frame"] == q["frame"] and t["n_total"] == q["n_total"] and _same(t["points"], q["points"])
    pl.close()


@pytest.mark.parametrize("sgm", [False, True])
@pytest.mark.parametrize("checked", [False, True])
@pytest.mark.parametrize("speckled", [False, True])
def test_all_eight_switch_combinations(rig, sgm, checked, speckled):
    S, c, L, Rr, cam = rig["S"], rig["ctx"], rig["L"], rig["R"], rig["cam"]
    pl = S.Pipeline(c, rig["pp"])
    pl.set_keyframe_clouds(True)
    if speckled:
        pl.set_keyframe_speckle_filter(*SPECKLE)
    if sgm:
        pl.set_keyframe_sgm()
    if checked:
        pl.set_keyframe_lr_check(MAX_DIFF)
    r = pl.process_batch(L[:1], Rr[:1])
    tab = pl.keyframe_clouds()
    assert r[0].is_keyframe == 1 and len(tab) == 1
    assert _same(tab[0]["points"], _want(("s0", 0), L[0], Rr[0], cam, sgm, checked, speckled))
    pl.close()


def test_group_clouds_are_those_of_the_sgm_maps_with_a_rectified_lane(ctx):
    """Session context (max_batch 4): 2 lanes x 2 frames per call, 3 calls; lane 1 is rectified (k1, p1) as in the group cloud test."""
    import torch
    import stereo_vo_amd as S
    from stereo_vo_amd import api
    lanes, batch, calls = 2, 2, 3
    n = batch * calls
    sub = api.SGM_KEYFRAME_SUB_BATCH
    seqs = [_seq(n, w=W, h=H, seed=0x5EED0A00 + 17 * i) for i in range(lanes)]
    p = seqs[0][0]
    pp = _params(S, p, MD)
    cam = S.CameraInfo(p.focal, p.cx, p.cy, 0, 0, 0, 0, p.baseline)
    eye = api.rectify_eye(p.focal, p.focal, p.cx, p.cy, k1=-0.03, p1=2e-4)
    Ls, Rs = np.stack([s[1] for s in seqs]), np.stack([s[2] for s in seqs])
    Lu = [Ls[0], np.stack([ctx.rectify_remap(x, eye, cam) for x in Ls[1]])]
    Ru = [Rs[0], np.stack([ctx.rectify_remap(x, eye, cam) for x in Rs[1]])]
    g = S.PipelineGroup(ctx, pp, lanes)
    g.set_rectification(1, eye, eye)
    with pytest.raises(S.SvoError, match="keyframe clouds are off"):
        g.set_keyframe_sgm()

    def run(sgm, filtered=False):
        out = [[] for _ in range(lanes)]
        seen = 0
        for b0 in range(0, n, batch):
            dl, dr = torch.from_numpy(Ls[:, b0:b0 + batch].copy()).cuda(), torch.from_numpy(Rs[:, b0:b0 + batch].copy()).cuda()
            res, launches = _launches(ctx, "stereo_sgm", lambda: g.process_batch_dev(dl.data_ptr(), dr.data_ptr(), batch * W * H, batch))
            torch.cuda.synchronize()
            for l in range(lanes):
                out[l] += [_bits(r) for r in res[l]]
            if sgm is None:
                assert launches == 0
                continue
            tab = g.keyframe_clouds()
            assert [(t["lane"], t["frame"]) for t in tab] == [(l, i) for l in range(lanes) for i in range(batch) if res[l][i].is_keyframe]
            assert launches == ((len(tab) + sub - 1) // sub if sgm else 0)
            for t in tab:
                l, f = t["lane"], b0 + t["frame"]
                want = _want(("g", l, f), Lu[l][f], Ru[l][f], cam, sgm, filtered, filtered)
                assert len(want) >= 1000 and t["n_total"] == len(want) and _same(t["points"], want), (sgm, filtered, l, f)
            seen += len(tab)
        return out, seen

    plain, _ = run(None)
    g.reset()
    g.set_keyframe_clouds(-1, True)
    with pytest.raises(S.SvoError, match="p2"):
        g.set_keyframe_sgm(5, 4)
    g.set_keyframe_sgm()
    got, seen = run(True)
    assert got == plain and seen == sum(b[4] for l in range(lanes) for b in plain[l]) >= lanes
    g.reset()
    g.set_keyframe_lr_check(MAX_DIFF)
    g.set_keyframe_speckle_filter(*SPECKLE)
    got, seen = run(True, True)
    assert got == plain and seen >= lanes
    # the group's carry-over: max_points one below the default means new buffers (every cloud is far below either bound), and
    # semi-global matching, the check and the speckle filter stay on: run() compares every cloud with the restatement of all three
    g.set_keyframe_clouds(-1, api.CloudParams(1, 0.0, W * H - 1), lanes * batch)
    g.reset()
    got, seen = run(True, True)
    assert got == plain and seen >= lanes
    g.reset()
    g.set_keyframe_sgm(on=False)
    got, seen = run(False, True)
    assert got == plain and seen >= lanes
    g.close()
