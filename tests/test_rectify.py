"""GPU: rectify_remap_kernel and the rectification entries (include/svo.h "rectification") against the declared integer
arithmetic restated in tests/rectify_ref.py, byte for byte; the pipelines fed RAW frames with a camera model against the
same pipelines fed the numpy-rectified frames, field for field.  (The reference has no counterpart: it carries k1..p2 in
CameraInfo, src/camera_info.hpp:10-14, and never reads them.)"""
import numpy as np
import pytest

import rectify_ref as RR
from test_pipeline import _seq

pytestmark = pytest.mark.gpu

SIZES = [(1241, 376), (61, 37), (64, 48), (1280, 720)]


def _cam(S, w, h):
    return S.CameraInfo(0.58 * w, 0.489 * w + 0.1928, 0.4926 * h + 0.2157, 0, 0, 0, 0, 0.54)


def _strong_model(S, w, h):
    """Barrel distortion + tangential terms + about 1 degree about each axis (border taps at the edges, sentinels at full size)."""
    from stereo_vo_amd import api
    cam = _cam(S, w, h)
    return cam, api.rectify_eye(cam.focal * 1.013, cam.focal * 0.991, cam.cx + 2.3, cam.cy - 1.7, -0.21, 0.06, 7e-4, -5e-4,
                                RR.rot(1.0, -1.1, 0.9))


def _zoom_model(S, w, h):
    """The raw camera sees 1 / 1.3 of the rectified field of view: a band without source (sentinels) and border taps around it."""
    from stereo_vo_amd import api
    cam = _cam(S, w, h)
    return cam, api.rectify_eye(cam.focal * 1.3, cam.focal * 1.27, cam.cx - 1.4, cam.cy + 0.9, 0.11, -0.03, -4e-4, 6e-4,
                                RR.rot(-0.8, 0.9, 1.1))


def _noise(w, h, seed, n=None):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (h, w) if n is None else (n, h, w), dtype=np.uint8)


def _mild_models(S, p):
    """Two stereo cameras, mild enough that the pipeline still tracks (checked on the CPU with the oracle pipeline on the
    numpy-rectified frames: keyframes at 4 or more frames of 12, at least 109 tracked features on every other frame)."""
    from stereo_vo_amd import api
    cam = S.CameraInfo(p.focal, p.cx, p.cy, 0, 0, 0, 0, p.baseline)
    A = (api.rectify_eye(p.focal * 1.004, p.focal * 0.997, p.cx + 1.3, p.cy - 0.8, -0.03, 0.008, 2e-4, -1e-4, RR.rot(0.15, -0.2, 0.1)),
         api.rectify_eye(p.focal * 0.998, p.focal * 1.003, p.cx - 0.9, p.cy + 0.6, -0.025, 0.006, -1e-4, 2e-4, RR.rot(-0.1, 0.15, -0.12)))
    B = (api.rectify_eye(p.focal * 0.996, p.focal * 1.002, p.cx - 1.1, p.cy + 0.7, 0.02, -0.005, -2e-4, 1e-4, RR.rot(-0.12, 0.1, 0.2)),
         api.rectify_eye(p.focal * 1.003, p.focal * 0.998, p.cx + 0.8, p.cy - 0.5, 0.024, -0.004, 1e-4, -2e-4, RR.rot(0.1, -0.1, -0.15)))
    return cam, A, B


def _ref_rectified(S, model, cam, L, R):
    w, h = L.shape[2], L.shape[1]
    ml = RR.build_map(RR.eye_dict(model[0]), RR.cam_dict(cam), w, h)
    mr = RR.build_map(RR.eye_dict(model[1]), RR.cam_dict(cam), w, h)
    return np.stack([RR.remap(x, ml) for x in L]), np.stack([RR.remap(x, mr) for x in R])


def _bits(r):
    """Every field of an svo_frame_result, floats as their bit patterns."""
    return (r.n_detected, r.n_tracked, r.n_inliers, r.n_new, r.is_keyframe, int(np.float32(r.av_parallax).view(np.uint32)),
            int(np.float32(r.percent_lost).view(np.uint32)), tuple(int(np.float64(v).view(np.uint64)) for v in r.pose7), r.ba_iterations)


def _params(S, p, md, maxc=600, mf=600):
    pp = S.pipeline_default_params()
    pp.cam.focal, pp.cam.cx, pp.cam.cy, pp.cam.baseline = p.focal, p.cx, p.cy, p.baseline
    pp.width, pp.height = p.width, p.height
    pp.max_corners, pp.min_feature_distance, pp.max_features = maxc, md, mf
    pp.ba_max_time_s = 0.0
    return pp


def _assert_not_vacuous(res):
    kf = [r.is_keyframe for r in res]
    assert kf[0] == 1 and sum(kf[1:]) >= 2, kf
    low = [(i, r.n_tracked) for i, r in enumerate(res) if not r.is_keyframe and r.n_tracked < 100]
    assert not low, low


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("model", ["strong", "zoom"])
def test_remap_equals_the_restatement_on_noise(ctx, w, h, model):
    import stereo_vo_amd as S
    cam, eye = (_strong_model if model == "strong" else _zoom_model)(S, w, h)
    m = RR.build_map(RR.eye_dict(eye), RR.cam_dict(cam), w, h)
    sent = m[..., 0] == RR.SENTINEL
    assert not sent.all() and (sent.any() or model == "strong")
    raw = _noise(w, h, 7 * w + h)
    got = ctx.rectify_remap(raw, eye, cam)
    exp = RR.remap(raw, m)
    assert np.array_equal(got, exp), int((got != exp).sum())
    assert not got[sent].any() and got[~sent].any()
    assert np.array_equal(np.ascontiguousarray(m), S.rectify_build_map(eye, cam, w, h))  # (the product's own table is the same one)


@pytest.mark.parametrize("w,h", [(1241, 376), (1280, 720)])
def test_remap_equals_the_restatement_on_synthetic_frames(ctx, w, h):
    import stereo_vo_amd as S
    cam, eye = _strong_model(S, w, h)
    m = RR.build_map(RR.eye_dict(eye), RR.cam_dict(cam), w, h)
    p = S.synth_default(w, h)
    for img in S.synth_render(p, 1):
        got = ctx.rectify_remap(img, eye, cam)
        assert np.array_equal(got, RR.remap(img, m))


@pytest.mark.parametrize("w,h,pad", [(1241, 376, 7), (61, 37, 3), (64, 48, 0), (1280, 720, 16)])
def test_remap_batch_dev_with_a_row_stride(ctx, w, h, pad):
    """Batch of 3, rows `pad` bytes apart from tight, images not tight either; output tight."""
    import torch
    import stereo_vo_amd as S
    cam, eye = _strong_model(S, w, h)
    m = RR.build_map(RR.eye_dict(eye), RR.cam_dict(cam), w, h)
    imgs = _noise(w, h, 11 * w + pad, n=3)
    if w == 1241:
        imgs[1] = S.synth_render(S.synth_default(w, h), 2)[0]
    stride = w + pad
    buf = np.full((3, h + 2, stride), 255, np.uint8)  # bytes beyond a row / an image must never be read as pixels
    buf[:, :h, :w] = imgs
    d_in = torch.from_numpy(buf).cuda()
    d_out = torch.full((3 * h * w + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    ctx.rectify_remap_batch_dev(d_in.data_ptr(), 3, w, h, stride, (h + 2) * stride, eye, cam, d_out.data_ptr())
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert np.all(out[3 * h * w:] == 0xAB)  # nothing written past the last image
    got = out[:3 * h * w].reshape(3, h, w)
    for i in range(3):
        assert np.array_equal(got[i], RR.remap(imgs[i], m)), i
    # the host entry with the same row stride
    assert np.array_equal(ctx.rectify_remap(buf[0, :h, :w], eye, cam), RR.remap(imgs[0], m))


@pytest.mark.parametrize("w,h", SIZES)
def test_identity_model_returns_the_input(ctx, w, h):
    import stereo_vo_amd as S
    cam = _cam(S, w, h)
    raw = _noise(w, h, w + 13 * h)
    assert np.array_equal(ctx.rectify_remap(raw, S.rectify_eye_from_camera_info(cam), cam), raw)


@pytest.mark.parametrize("w,h", SIZES)
def test_shift_model_returns_the_shifted_image(ctx, w, h):
    """Raw principal point at (+3, -2): out(v, u) = raw(v - 2, u + 3), zero where that is outside (numpy slices, no restatement)."""
    import stereo_vo_amd as S
    from stereo_vo_amd import api
    cam = _cam(S, w, h)
    raw = _noise(w, h, 3 * w + h)
    got = ctx.rectify_remap(raw, api.rectify_eye(cam.focal, cam.focal, cam.cx + 3.0, cam.cy - 2.0), cam)
    exp = np.zeros_like(raw)
    exp[2:, :w - 3] = raw[:h - 2, 3:]
    assert np.array_equal(got, exp)


# ------------------------------------------------------------------------------------------------ single pipeline
@pytest.mark.parametrize("w,h,focal,md", [(496, 160, 300.0, 10.0), (1241, 376, 718.856, 14.0)])
def test_pipeline_on_raw_frames_equals_pipeline_on_rectified_frames(w, h, focal, md):
    import stereo_vo_amd as S
    n = 12
    p, L, R = _seq(n, w=w, h=h, focal=focal, seed=0x5EED0A00)
    cam, A, _ = _mild_models(S, p)
    Lr, Rr = _ref_rectified(S, A, cam, L, R)
    assert (Lr != L).mean() > 0.2  # the model does something
    c = S.Context(w, h, max_batch=n, max_corners=600, max_candidates=1 << 17, max_features=600)
    pp = _params(S, p, md)
    # run B: no rectification, numpy-rectified frames
    b = S.Pipeline(c, pp)
    res_b = b.process_batch(Lr, Rr)
    ids_b, xy_b = b.tracked()
    _assert_not_vacuous(res_b)
    # ... and what the raw frames give WITHOUT the model (today's behaviour), for the turn-off check below
    b.reset()
    res_raw = b.process_batch(L, R)
    assert [_bits(r) for r in res_raw] != [_bits(r) for r in res_b]
    # run A: rectification set, raw frames; in two batches, through the host entry and the device-pointer entry
    import torch
    a = S.Pipeline(c, pp)
    a.set_rectification(A[0], A[1])
    res_a = a.process_batch(L[:5], R[:5])
    dl, dr = torch.from_numpy(L[5:].copy()).cuda(), torch.from_numpy(R[5:].copy()).cuda()
    res_a += a.process_batch_dev(dl.data_ptr(), dr.data_ptr(), n - 5)
    torch.cuda.synchronize()
    ids_a, xy_a = a.tracked()
    for i in range(n):
        assert _bits(res_a[i]) == _bits(res_b[i]), (i, _bits(res_a[i]), _bits(res_b[i]))
    assert np.array_equal(ids_a, ids_b) and np.array_equal(xy_a.view(np.uint32), xy_b.view(np.uint32)) and len(ids_a) >= 100
    # off again on the same object: today's results on the raw frames
    a.set_rectification(None, None)
    a.reset()
    res_off = a.process_batch(L, R)
    assert [_bits(r) for r in res_off] == [_bits(r) for r in res_raw]
    a.close()
    b.close()
    c.close()


# ------------------------------------------------------------------------------------------------ group
def test_group_lanes_with_different_cameras_equal_their_single_pipelines():
    """Three lanes: lane 0 camera A, lane 1 none, lane 2 camera B.  Device-pointer entry, streaming entry (both slots, three
    batches) and the copying entry: every lane == its own single pipeline, lane 1 == the lane of a group without any model."""
    import torch
    import stereo_vo_amd as S
    n, lanes, batch, md = 12, 3, 4, 10.0
    w, h = 496, 160
    seqs = [_seq(n, w=w, h=h, seed=0x5EED0A00 + 17 * i) for i in range(lanes)]
    p = seqs[0][0]
    cam, A, B = _mild_models(S, p)
    model = [A, None, B]
    Ls, Rs = np.stack([s[1] for s in seqs]), np.stack([s[2] for s in seqs])
    c = S.Context(w, h, max_batch=lanes * batch, max_corners=600, max_candidates=1 << 17, max_features=600)
    pp = _params(S, p, md)

    # what every lane must give: its own single pipeline, raw frames + its model (none for lane 1)
    want = []
    for l in range(lanes):
        s = S.Pipeline(c, pp)
        if model[l]:
            s.set_rectification(*model[l])
        res = []
        for b0 in range(0, n, batch):
            res += s.process_batch(Ls[l, b0:b0 + batch], Rs[l, b0:b0 + batch])
        want.append(([_bits(r) for r in res], s.tracked()))
        if model[l]:  # ... which is the pipeline on the numpy-rectified frames (the previous test's run B), and not vacuous
            Lr, Rr = _ref_rectified(S, model[l], cam, Ls[l], Rs[l])
            s.set_rectification(None, None)
            s.reset()
            rb = s.process_batch(Lr[:batch], Rr[:batch]) + s.process_batch(Lr[batch:2 * batch], Rr[batch:2 * batch]) + \
                s.process_batch(Lr[2 * batch:], Rr[2 * batch:])
            _assert_not_vacuous(rb)
            assert [_bits(r) for r in rb] == want[l][0], l
        s.close()

    g = S.PipelineGroup(c, pp, lanes)

    def dev_run(bsz):
        out = [[] for _ in range(lanes)]
        for b0 in range(0, n, bsz):
            dl, dr = torch.from_numpy(Ls[:, b0:b0 + bsz].copy()).cuda(), torch.from_numpy(Rs[:, b0:b0 + bsz].copy()).cuda()
            res = g.process_batch_dev(dl.data_ptr(), dr.data_ptr(), bsz * w * h, bsz)
            torch.cuda.synchronize()
            for l in range(lanes):
                out[l] += res[l]
        return [[_bits(r) for r in o] for o in out]

    def check(got, what):
        for l in range(lanes):
            assert got[l] == want[l][0], (what, l)
            ig, xg = g.get_tracked(l)
            assert np.array_equal(ig, want[l][1][0]) and np.array_equal(xg.view(np.uint32), want[l][1][1].view(np.uint32)), (what, l)

    plain = dev_run(batch)  # no lane has a model: today's group
    assert plain[1] == want[1][0]
    g.reset()
    g.set_rectification(0, *A)
    g.set_rectification(2, *B)
    # (1) device-pointer entry
    got = dev_run(batch)
    check(got, "process_batch_dev")
    assert got[1] == plain[1] and got[0] != plain[0] and got[2] != plain[2]
    # (2) streaming: fill the other slot and start its upload, then process this one
    g.reset()
    got = [[] for _ in range(lanes)]
    nb = n // batch
    sl, sr = g.staging(0)
    sl[:, :batch], sr[:, :batch] = Ls[:, :batch], Rs[:, :batch]
    g.upload(0, batch)
    for b in range(nb):
        if b + 1 < nb:
            nl, nr = g.staging((b + 1) & 1)
            nl[:, :batch], nr[:, :batch] = Ls[:, (b + 1) * batch:(b + 2) * batch], Rs[:, (b + 1) * batch:(b + 2) * batch]
            g.upload((b + 1) & 1, batch)
        res = g.process_uploaded(b & 1, batch)
        for l in range(lanes):
            got[l] += [_bits(r) for r in res[l]]
    check(got, "streaming")
    # (3) the copying entry, batches shorter than the slots
    g.reset()
    got = [[] for _ in range(lanes)]
    for b0 in range(0, n, 3):
        res = g.process_batch(Ls[:, b0:b0 + 3], Rs[:, b0:b0 + 3])
        for l in range(lanes):
            got[l] += [_bits(r) for r in res[l]]
    check(got, "process_batch")
    # (4) every lane the same camera (lane = -1): the contiguous workspace; lanes 0 and 2 as a single pipeline with camera A
    g.reset()
    g.set_rectification(-1, *A)
    got = dev_run(batch)
    assert got[0] == want[0][0]
    s = S.Pipeline(c, pp)
    s.set_rectification(*A)
    for l in (1, 2):
        s.reset()
        assert got[l] == [_bits(r) for r in s.process_batch(Ls[l], Rs[l])], l
    s.close()
    # (5) off again: today's results on the same object after a reset
    g.set_rectification(-1, None, None)
    g.reset()
    assert dev_run(batch) == plain
    g.close()
    c.close()
