"""GPU: the left-right check between the dense launch and the speckle filter / the clouds of a pipeline and of a pipeline group
(include/svo.h, svo_pipeline_set_keyframe_lr_check and the group's form).  Every keyframe's cloud equals the triangulation of the
restatement-checked oracle map (tests/lr_check_ref.py::check_arrays over oracle StereoBM(48, 21), cost from lr_check_ref.min_sad,
then speckle_ref.filter_propagate when the speckle filter is on as well), bit for bit; the frame results and the tracked set are
those of a run with nothing on; turning the check off restores the unchecked clouds.

max_diff16 = 16 (disp12MaxDiff = 1 pixel), fixed on the CPU with the restatement alone before any device run: on every frame of
both streams the check removes at least one pixel and leaves far more than 1,000.  Removed / valid pixels of the oracle maps per
frame (the keyframes are frames 0, 4, 7 and 10 of the pipeline's stream and frames 0 and 4 of each lane of the group, whose
rectified lane 1 loses 73 / 44,869 and 85 / 47,018):
  stream 0x5EED0A00, frames 0..11: 73 / 44,112  95 / 45,199  112 / 45,710  189 / 46,640  252 / 47,715  352 / 48,930  515 / 50,634
                                   378 / 51,317  465 / 52,108  612 / 52,993  365 / 52,805  1,583 / 45,484
  stream 0x5EED0A11 (the group's lane 1 before rectification), frames 0..5: 75 / 44,293  28 / 44,583  38 / 44,933  39 / 45,484
                                   86 / 46,141  224 / 47,112
(max_diff16 = 0 removes 953 to 2,874 per frame; it was not needed.)"""
import numpy as np
import pytest

import lr_check_ref as LR
import oracle_lib as O
import speckle_ref as SP
from test_dense_cloud import _expected_cloud, _same
from test_dense_cloud_pipeline import CALL, H, MD, N, W, _run
from test_pipeline import _seq
from test_rectify import _bits, _params

pytestmark = pytest.mark.gpu

MAX_DIFF = 16
SPECKLE = (100, 32)
_MAPS = {}


def _want(key, left, right, cam, checked, speckled=False):
    """(expected cloud, pixels the check removed) of one rectified pair; the maps of a pair are formed once per session (`key`)."""
    if key not in _MAPS:
        m = O.stereo_bm(left, right, 48, 21)
        out, n = LR.check_arrays(m, LR.min_sad(left, right, 48, 21), MAX_DIFF)
        _MAPS[key] = (m, out, n, {})
    m, out, n, sp = _MAPS[key]
    use = out if checked else m
    if speckled:
        if checked not in sp:
            sp[checked] = SP.filter_propagate(use, *SPECKLE)[0]
        use = sp[checked]
    return _expected_cloud(left, use, cam, 1, 0.0, None), (n if checked else 0)


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


@pytest.mark.parametrize("speckled", [False, True], ids=["check", "check_and_speckle"])
def test_pipeline_clouds_are_those_of_the_checked_maps(rig, speckled):
    S, c, L, Rr, cam = rig["S"], rig["ctx"], rig["L"], rig["R"], rig["cam"]
    pl = S.Pipeline(c, rig["pp"])
    # ordering: the check before the clouds is a loud error, and nothing is on afterwards
    with pytest.raises(S.SvoError, match="keyframe clouds are off"):
        pl.set_keyframe_lr_check(MAX_DIFF)
    pl.set_keyframe_clouds(True)
    with pytest.raises(S.SvoError, match="max_diff16"):
        pl.set_keyframe_lr_check(-1)
    if speckled:  # the two switches are independent: either order
        pl.set_keyframe_speckle_filter(*SPECKLE)
    pl.set_keyframe_lr_check(MAX_DIFF)
    res, seen = [], 0
    for b0 in range(0, N, CALL):
        c.profile_select("lr_check")
        r = pl.process_batch(L[b0:b0 + CALL], Rr[b0:b0 + CALL])
        launches = c.profile_read()[1]
        c.profile_select(None)
        res += r
        tab = pl.keyframe_clouds()
        assert [t["frame"] for t in tab] == [i for i, x in enumerate(r) if x.is_keyframe]
        assert launches == (1 if tab else 0)
        for t in tab:
            f = b0 + t["frame"]
            want, n = _want(("s0", f), L[f], Rr[f], cam, True, speckled)
            plain, _ = _want(("s0", f), L[f], Rr[f], cam, False, speckled)
            print("keyframe", f, "removed by the check", n, "points", len(want), "without the check", len(plain))
            assert n >= 1 and len(want) >= 1000 and not _same(want, plain), (f, n, len(want))
            assert t["n_total"] == t["n_stored"] == len(want) and _same(t["points"], want), (b0, t["frame"])
            seen += 1
    assert seen == sum(x.is_keyframe for x in res) >= 2
    # svo_frame_result and the tracked set: those of the run with nothing on
    assert [_bits(x) for x in res] == [_bits(x) for x in rig["res"]]
    ids, xy = pl.tracked()
    assert np.array_equal(ids, rig["tracked"][0]) and np.array_equal(xy.view(np.uint32), rig["tracked"][1].view(np.uint32))
    # new cloud parameters keep the check (and the speckle filter)
    from stereo_vo_amd import api
    pl.set_keyframe_clouds(api.CloudParams(1, 0.0, W * H), 2)
    pl.reset()
    r = pl.process_batch(L[:1], Rr[:1])
    tab = pl.keyframe_clouds()
    assert r[0].is_keyframe == 1 and len(tab) == 1 and _same(tab[0]["points"], _want(("s0", 0), L[0], Rr[0], cam, True, speckled)[0])
    # off again: the unchecked clouds, no launch, the speckle filter as it was
    pl.set_keyframe_lr_check(None)
    pl.reset()
    c.profile_select("lr_check")
    r = pl.process_batch(L[:CALL], Rr[:CALL])
    launches = c.profile_read()[1]
    c.profile_select(None)
    tab = pl.keyframe_clouds()
    assert launches == 0 and tab
    for t in tab:
        f = t["frame"]
        want = _want(("s0", f), L[f], Rr[f], cam, False, speckled)[0]
        assert t["n_total"] == len(want) and _same(t["points"], want)
        if not speckled:
            alone, n_total = c.stereo_cloud(L[f], Rr[f], cam)
            assert n_total == len(want) and _same(alone, want)
    # clouds off frees the check with them: turning it on again needs the clouds first
    pl.set_keyframe_lr_check(MAX_DIFF)
    pl.set_keyframe_clouds(None)
    with pytest.raises(S.SvoError, match="keyframe clouds are off"):
        pl.set_keyframe_lr_check(MAX_DIFF)
    pl.close()


def test_group_clouds_are_those_of_the_checked_maps_with_a_rectified_lane(ctx):
    """Session context (max_batch 4): 2 lanes x 2 frames per call, 3 calls; lane 1 is rectified (k1, p1) as in the group cloud test."""
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
    Lu = [Ls[0], np.stack([ctx.rectify_remap(x, eye, cam) for x in Ls[1]])]
    Ru = [Rs[0], np.stack([ctx.rectify_remap(x, eye, cam) for x in Rs[1]])]
    g = S.PipelineGroup(ctx, pp, lanes)
    g.set_rectification(1, eye, eye)
    with pytest.raises(S.SvoError, match="keyframe clouds are off"):
        g.set_keyframe_lr_check(MAX_DIFF)

    def run(checked, speckled=False):
        out = [[] for _ in range(lanes)]
        seen = 0
        for b0 in range(0, n, batch):
            dl, dr = torch.from_numpy(Ls[:, b0:b0 + batch].copy()).cuda(), torch.from_numpy(Rs[:, b0:b0 + batch].copy()).cuda()
            ctx.profile_select("lr_check")
            res = g.process_batch_dev(dl.data_ptr(), dr.data_ptr(), batch * W * H, batch)
            launches = ctx.profile_read()[1]
            ctx.profile_select(None)
            torch.cuda.synchronize()
            for l in range(lanes):
                out[l] += [_bits(r) for r in res[l]]
            if checked is None:
                assert launches == 0
                continue
            tab = g.keyframe_clouds()
            assert [(t["lane"], t["frame"]) for t in tab] == [(l, i) for l in range(lanes) for i in range(batch) if res[l][i].is_keyframe]
            assert launches == (1 if tab and checked else 0)
            for t in tab:
                l, f = t["lane"], b0 + t["frame"]
                want, nrem = _want(("g", l, f), Lu[l][f], Ru[l][f], cam, checked, speckled)
                print("lane", l, "frame", f, "removed by the check", nrem, "points", len(want))
                assert (nrem >= 1) == checked and len(want) >= 1000
                assert t["n_total"] == len(want) and _same(t["points"], want), (checked, speckled, l, f)
            seen += len(tab)
        return out, seen

    plain, _ = run(None)
    g.reset()
    g.set_keyframe_clouds(-1, True)
    with pytest.raises(S.SvoError, match="max_diff16"):
        g.set_keyframe_lr_check(-1)
    g.set_keyframe_lr_check(MAX_DIFF)
    got, seen = run(True)
    assert got == plain and seen == sum(b[4] for l in range(lanes) for b in plain[l]) >= lanes
    g.reset()
    g.set_keyframe_speckle_filter(*SPECKLE)
    got, seen = run(True, True)
    assert got == plain and seen >= lanes
    g.reset()
    g.set_keyframe_lr_check(None)
    got, seen = run(False, True)
    assert got == plain and seen >= lanes
    g.reset()
    g.set_keyframe_speckle_filter(None)
    got, seen = run(False)
    assert got == plain and seen >= lanes
    g.close()
