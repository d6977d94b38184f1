"""CPU: svo_rectify_build_map (host only, no GPU) against the float64 restatement tests/rectify_ref.py, element for element,
plus known answers that do not go through the restatement, the sentinels and the int16 overflow error."""
import ctypes as C

import numpy as np
import pytest

import rectify_ref as RR
import stereo_vo_amd as S
from stereo_vo_amd import api

SIZES = [(1241, 376), (61, 37), (64, 48), (1280, 720)]


def _cam(w, h, focal=None):
    focal = 0.58 * w if focal is None else focal
    return S.CameraInfo(focal, 0.489 * w + 0.1928, 0.4926 * h + 0.2157, 0, 0, 0, 0, 0.54)


def _models(w, h):
    cam = _cam(w, h)
    barrel = api.rectify_eye(cam.focal * 1.013, cam.focal * 0.991, cam.cx + 2.3, cam.cy - 1.7, -0.21, 0.06, 7e-4, -5e-4,
                             RR.rot(1.0, -1.1, 0.9))
    pincushion = api.rectify_eye(cam.focal * 0.985, cam.focal * 1.007, cam.cx - 1.9, cam.cy + 2.6, 0.17, -0.04, -6e-4, 8e-4,
                                 RR.rot(-0.9, 1.0, -1.2))
    return cam, {"barrel": barrel, "pincushion": pincushion}


def _both(eye, cam, w, h):
    got = S.rectify_build_map(eye, cam, w, h)
    exp = RR.build_map(RR.eye_dict(eye), RR.cam_dict(cam), w, h)
    return got, exp


@pytest.mark.parametrize("w,h", SIZES)
def test_identity_model_is_all_zero(w, h):
    cam = _cam(w, h)
    eye = S.rectify_eye_from_camera_info(cam)
    got, exp = _both(eye, cam, w, h)
    assert np.array_equal(got, exp)
    assert not got.any()


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("which", ["barrel", "pincushion"])
def test_distorted_rotated_models_match_the_restatement(w, h, which):
    cam, models = _models(w, h)
    got, exp = _both(models[which], cam, w, h)
    assert got.dtype == np.int16 and got.shape == (h, w, 2)
    assert np.array_equal(got, exp), int((got != exp).sum())
    inside = got[..., 0] != RR.SENTINEL
    assert inside.mean() > 0.5 and np.abs(got[inside]).max() > 32  # not vacuous: most pixels have a source, and it is a real warp


def test_shifted_principal_point_known_answer():
    w, h = 1241, 376
    cam = _cam(w, h)
    eye = api.rectify_eye(cam.focal, cam.focal, cam.cx + 3.0, cam.cy - 2.0)
    got = S.rectify_build_map(eye, cam, w, h)
    inside = got[..., 0] != RR.SENTINEL
    assert np.all(got[inside] == np.array([96, -64], np.int16))
    # the source (u + 3, v - 2) has a tap in the image for u <= w - 4 (ix = u + 3 <= w - 1) and v >= 1 (iy = v - 2 >= -1)
    exp_inside = np.zeros((h, w), bool)
    exp_inside[1:, :w - 3] = True
    assert np.array_equal(inside, exp_inside)
    assert np.all(got[~inside] == RR.SENTINEL)


def test_doubled_focal_known_answer():
    w, h = 64, 48
    cam = S.CameraInfo(40.0, 31.5, 23.25, 0, 0, 0, 0, 0.5)
    eye = api.rectify_eye(80.0, 80.0, cam.cx, cam.cy)
    got = S.rectify_build_map(eye, cam, w, h)
    inside = got[..., 0] != RR.SENTINEL
    u = np.arange(w)[None, :].repeat(h, 0)
    v = np.arange(h)[:, None].repeat(w, 1)
    # source = c + 2 (p - c): dx = 32 (u - cx) = 32 u - 1008, dy = 32 (v - cy) = 32 v - 744, integers everywhere
    assert inside.any()
    assert np.array_equal(got[..., 0][inside], (32 * u - 1008)[inside])
    assert np.array_equal(got[..., 1][inside], (32 * v - 744)[inside])
    # a tap is inside iff -1 <= 2 u - 31.5 (floor) <= w - 1
    ix = np.floor(2 * u - 31.5)
    iy = np.floor(2 * v - 23.25)
    assert np.array_equal(inside, (ix >= -1) & (ix <= w - 1) & (iy >= -1) & (iy <= h - 1))


def test_border_band_outside_the_raw_image_is_sentinel():
    w, h = 64, 48
    cam = S.CameraInfo(40.0, 31.5, 23.5, 0, 0, 0, 0, 0.5)
    eye = api.rectify_eye(60.0, 60.0, cam.cx, cam.cy)  # zoom 1.5: the outer band of the rectified image has no source
    got, exp = _both(eye, cam, w, h)
    assert np.array_equal(got, exp)
    sent = (got[..., 0] == RR.SENTINEL) & (got[..., 1] == RR.SENTINEL)
    assert sent[0].all() and sent[-1].all() and sent[:, 0].all() and sent[:, -1].all()
    assert not sent[h // 2, w // 2] and 0.3 < sent.mean() < 0.8
    assert not ((got[..., 0] == RR.SENTINEL) ^ (got[..., 1] == RR.SENTINEL)).any()


def test_points_behind_the_raw_camera_are_sentinel():
    w, h = 64, 48
    cam = S.CameraInfo(40.0, 31.5, 23.5, 0, 0, 0, 0, 0.5)
    # W = (R[2] xn + R[5] yn) + R[8] with R = rotation by 180 degrees about y: W = -1 everywhere
    eye = api.rectify_eye(40.0, 40.0, cam.cx, cam.cy, R=[-1, 0, 0, 0, 1, 0, 0, 0, -1])
    got, exp = _both(eye, cam, w, h)
    assert np.array_equal(got, exp)
    assert np.all(got == RR.SENTINEL)
    # ... and a rotation of 60 degrees about y puts W = 0 across the image: one side has a source candidate, the other none
    eye = api.rectify_eye(40.0, 40.0, cam.cx, cam.cy, R=RR.rot(0, 60, 0))
    got, exp = _both(eye, cam, w, h)
    assert np.array_equal(got, exp)
    xn = (np.arange(w) - cam.cx) / cam.focal
    Wd = np.asarray(RR.rot(0, 60, 0)).reshape(-1)[2] * xn + np.asarray(RR.rot(0, 60, 0)).reshape(-1)[8]
    assert (Wd <= 0).any() and np.all(got[:, Wd <= 0] == RR.SENTINEL)


def test_displacement_beyond_int16_is_an_error_with_a_message():
    w, h = 1280, 720
    cam = _cam(w, h)
    eye = api.rectify_eye(cam.focal, cam.focal, cam.cx + 1100.0, cam.cy)  # 1100 px > 32767 / 32 px, sources still inside on the left
    out = np.empty((h, w, 2), np.int16)
    rc = S.lib().svo_rectify_build_map(C.byref(eye), C.byref(cam), w, h, out.ctypes.data_as(C.c_void_p))
    assert rc == -1  # SVO_ERR_INVALID
    msg = S.lib().svo_last_error(None).decode()
    assert "int16" in msg and "displacement" in msg, msg
    with pytest.raises(RR.DisplacementOverflow):
        RR.build_map(RR.eye_dict(eye), RR.cam_dict(cam), w, h)
    # 1000 px fits
    eye = api.rectify_eye(cam.focal, cam.focal, cam.cx + 1000.0, cam.cy)
    got, exp = _both(eye, cam, w, h)
    assert np.array_equal(got, exp) and (got[..., 0] == 32000).any()


def test_eye_from_camera_info_round_trips_the_fields():
    cam = S.CameraInfo(718.856, 607.1928, 185.2157, -0.3, 0.1, 1e-3, -2e-3, 0.537)
    e = S.rectify_eye_from_camera_info(cam)
    assert (e.fx, e.fy, e.cx, e.cy) == (cam.focal, cam.focal, cam.cx, cam.cy)
    assert (e.k1, e.k2, e.p1, e.p2) == (cam.k1, cam.k2, cam.p1, cam.p2)
    assert list(e.R) == [1, 0, 0, 0, 1, 0, 0, 0, 1]
    assert S.lib().svo_rectify_eye_from_camera_info(None, C.byref(e)) == -1
