"""a2/a3/a4 pyramid, pyrLK and the survivor filter on scenes that reach every decision, judged by an independent restatement
(tests/lk_ref.py).

`tests/test_frontend.py` compares the kernel with the oracle on one mild synthetic stream and four smoothed-noise shifts; the
oracle shares the kernel's structure.  Here the scenes are built for the decisions (windows outside a level, flat levels, a
window that leaves in mid-iteration, the three loop exits, weight ties, sums beyond int32, borders, restaging, the survivor
filter at its thresholds and at the block sizes of the compaction), the restatement counts them, and both the oracle (CPU) and
`svo_lk_track` / `svo_track_features` / `svo_build_pyramid` (GPU) must return its bytes.

The CPU part (oracle = restatement on 37 scenes and 7 pyramids, counters, 11 mutations) takes 13 s of wall time, measured;
the searches that found the points of FINAL_OUT and BAND (130 s and 28 s) are not part of it.
"""
import functools
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import lk_ref as R

F = np.float32
FAR = np.array([[1e5, 5.0], [-1e5, 5.0], [5.0, 1e5], [5.0, -1e5], [1048575.0, -1048575.0], [-300.5, 4.25], [4.25, 400.5]], F)


# ----------------------------------------------------------------------------------------------------------------- scenes
def canvas(seed, w, h, cell, smooth, margin=72):
    """Block noise (cells of `cell` px) under `smooth` passes of [1 2 1] / 4, as float64, `margin` px larger on every side."""
    rng = np.random.default_rng(seed)
    H, W = h + 2 * margin, w + 2 * margin
    big = np.kron(rng.integers(0, 256, (H // cell + 1, W // cell + 1)).astype(np.float64), np.ones((cell, cell)))[:H, :W]
    for _ in range(smooth):
        big[:, 1:-1] = (big[:, :-2] + 2 * big[:, 1:-1] + big[:, 2:]) / 4
        big[1:-1, :] = (big[:-2, :] + 2 * big[1:-1, :] + big[2:, :]) / 4
    return big


def view(big, w, h, dx, dy, margin=72):
    """The w x h view of the canvas whose content is displaced by (dx, dy), bilinear, rounded to uint8."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    x, y = xx + margin - dx, yy + margin - dy
    x0, y0 = np.floor(x).astype(int), np.floor(y).astype(int)
    fx, fy = x - x0, y - y0
    v = (big[y0, x0] * (1 - fx) * (1 - fy) + big[y0, x0 + 1] * fx * (1 - fy) + big[y0 + 1, x0] * (1 - fx) * fy +
         big[y0 + 1, x0 + 1] * fx * fy)
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def grid(w, h, nx, ny, out=23.0):
    """nx x ny points from `out` px outside the top-left to `out` px outside the bottom-right corner, at odd fractions."""
    gx, gy = np.meshgrid(np.linspace(-out + 0.3, w + out - 0.45, nx), np.linspace(-out + 0.15, h + out - 0.7, ny))
    return np.stack([gx.ravel(), gy.ravel()], 1).astype(F)


def scene(A, B, xy, init=None):
    xy = np.ascontiguousarray(xy, F).reshape(-1, 2)
    init = xy.copy() if init is None else np.ascontiguousarray(init, F).reshape(-1, 2)
    assert A.shape == B.shape and A.dtype == B.dtype == np.uint8 and len(init) == len(xy)
    assert np.isfinite(xy).all() and np.isfinite(init).all() and np.abs(xy).max(initial=0) < 2 ** 20
    return dict(A=np.ascontiguousarray(A), B=np.ascontiguousarray(B), xy=xy, init=init)


def shifted(seed, w, h, shift, pts, cell=3, smooth=1):
    big = canvas(seed, w, h, cell, smooth)
    return scene(view(big, w, h, 0, 0), view(big, w, h, *shift), pts)


def size_scene(w, h, shift, nx, ny, extra=()):
    pts = np.concatenate([grid(w, h, nx, ny), border_ring(w, h), FAR] + [np.asarray(e, F).reshape(-1, 2) for e in extra])
    return shifted(1000 * w + h, w, h, shift, pts)


def border_ring(w, h):
    """Points 21, 11, 10 and 1 px outside each border and on it (the template test turns at -11 and w + 10, the window at -21)."""
    out = []
    for d in (21.5, 21.0, 11.25, 11.0, 10.75, 10.0, 1.0, 0.0):
        out += [(-d, h / 2), (w - 1 + d, h / 2), (w / 2, -d), (w / 2, h - 1 + d)]
    return np.array(out, F)


def tile_edge_points(w, h):
    """Level-0 templates whose 24 x 24 source tile (top-left = floor(p - 10) - 1) ends at w, one column short of it and one
    beyond it, the other axis inside; the same for rows."""
    pts = []
    for d in (-1, 0, 1):
        pts.append((w + d - 13 + 0.37, min(h - 14, 12) + 0.61))
        pts.append((min(w - 14, 12) + 0.37, h + d - 13 + 0.61))
    return np.array(pts, F)


def nyquist_pair(w, h):
    """128 + (-1)^x g(y) + (-1)^y k(x) with g and k triangle waves of period 8 and amplitude 60: textured at level 0 (both
    derivatives alive), while pyrDown's [1 4 6 4 1] has its zero at exactly this frequency, so levels 1 to 3 are all but
    constant.  The second image is the same function two pixels further in both axes (parity kept)."""
    def tri(n, phase):
        return (60 * (1 - 4 * np.abs(((np.arange(n) + phase) % 8) / 8 - 0.5))).astype(np.int64)
    g, k = tri(h + 8, 0), tri(w + 8, 3)

    def img(o):
        y, x = np.mgrid[0:h, 0:w]
        return (128 + np.where(x % 2, -1, 1) * g[y + o] + np.where(y % 2, -1, 1) * k[x + o]).astype(np.uint8)
    return img(0), img(2)


def blocks_pair(w, h):
    """0 / 255 stripes of period 4 in x whose phase turns over every 4 rows (period 8 in y), and the complement.  (2 x 2
    blocks of period 4 in BOTH axes have |Ix| = |Iy| = 2550 at every pixel: 441 * 2550^2 = 2.87e9 stays below 2^32; here half
    the rows have |Ix| = 4080.)"""
    y, x = np.mgrid[0:h, 0:w]
    A = np.where((x % 4 < 2) ^ (y % 8 < 4), 255, 0).astype(np.uint8)
    return A, (255 - A).astype(np.uint8)


def fb_exact_pair(w=64, h=48, px=32, y0=24, m=5):
    """A pair on which the forward pass moves a point at (px, y0 + 4 k) by exactly (-2, 0) and the backward pass does not move
    it at all, so that |old - back| is exactly 2.  Every quantity is an integer and every f32 product of the solve is exact:
      A = f(x) + (-1)^y r(y): f a ramp of slope m under the windows, r a triangle wave of slope 8 and period 8 that is
          symmetric about y0.  Ix = 32 m and Iy = 16 (q(y + 1) - q(y - 1)) = +-256 or 0, with sum 0 over any window centred on a
          peak or trough: A12 = 0 and b2 = 0.  pyrDown all but removes (-1)^y r(y): levels 1 to 3 have minEig < 0.01 and are skipped.
      B = A + e(x), e = 2 m except e(px - 13) = 34 m, e(px + 9) = -8 m, e(px + 10) = 12 m.
    Forward, iteration 0 at px: sum of e over [px - 10, px + 10] is 42 m, b1 = 2 A11, step -2 (= -fl(2 P fl(1 / P)), P = A11 A22);
    iteration 1 at px - 2: B(x - 2) = A(x) on the whole window, step 0.  Backward from px - 2, template B on [px - 12, px + 8]:
    sum of e(x) (2 m + e(x + 1) - e(x - 1)) = 19 * 4 m^2 - 60 m^2 (at px - 12) - 16 m^2 (at px + 8) = 0, so b1 = 0: step 0."""
    y, x = np.mgrid[0:h, 0:w]
    f = 40 + m * np.clip(x - (px - 14), 0, 26)
    r = 8 * np.abs(((y - y0) % 8) - 4)
    A = f + np.where(y % 2, -1, 1) * r
    e = np.full(w, 2 * m)
    e[px - 13] += 32 * m
    e[px + 9] -= 10 * m
    e[px + 10] += 10 * m
    B = A + e[x]
    assert A.min() >= 0 and B.min() >= 0 and A.max() <= 255 and B.max() <= 255
    return A.astype(np.uint8), B.astype(np.uint8)


def count_scene(n):
    """n features of which every 37th (and the last) is a real one on a small textured pair; the rest lie far outside the
    image (status 0 at once).  The kept ones are spread over every 1024- and 4096-block of the compaction."""
    w, h = 72, 56
    big = canvas(77, w, h, 3, 1)
    A, B = view(big, w, h, 0, 0), view(big, w, h, 0.8, -0.6)
    rng = np.random.default_rng(n)
    i = np.arange(n)
    xy = np.stack([-5000.0 - i, 7000.0 + 3 * i], 1).astype(F)
    real = (i % 37 == 0) | (i == n - 1)
    xy[real] = rng.uniform((8, 8), (w - 8, h - 8), (int(real.sum()), 2)).astype(F)
    init = xy + rng.uniform(-3, 3, xy.shape).astype(F)
    return scene(A, B, xy, init)


# Found by a search kept out of the suite (restatement over seeds 60..89 of canvas(), 160 points along the four borders per
# pair): level-0 loops that end by a rule of their own and whose LAST step carries the window out of [-21, w) x [-21, h), so
# that only the final bounds check clears the status.  name -> (seed, shift, cell, smooth, point)
FINAL_OUT = {
    "final_out_cap_left": (60, (-9.0, -9.0), 1, 0, (-4.864343166351318, 11.71733570098877)),
    "final_out_cap_bottom": (65, (12.0, 3.0), 6, 2, (63.823814392089844, 75.716796875)),
    "final_out_right": (86, (7.0, 0.0), 6, 2, (98.10669708251953, 27.1053524017334)),
    "final_out_cap_right": (80, (-9.0, -9.0), 1, 0, (102.83789825439453, 23.893461227416992)),
}
# Found the same way (seeds 100..170, 250 random points per pair, 28 s): a step whose dx^2 + dy^2 lies within 1e-4 relative of
# eps^2 = 1e-4, where the kernel leaves its f32 test for the reference's f64 expression.  name -> (seed, shift, point)
BAND = {
    "band_stop_a": (110, (1.29, 0.04), (59.34590530395508, 12.603519439697266)),
    "band_stop_b": (148, (0.41, 0.15), (62.97022247314453, 47.99167251586914)),
    "band_go_a": (127, (-1.31, -0.87), (39.12078857421875, 40.04935073852539)),
    "band_go_b": (137, (1.07, -0.67), (60.83898162841797, 16.534204483032227)),
}
COUNTS = (1, 63, 64, 65, 1023, 1024, 1025, 4096, 4097, 8200)
SIZES = ((8, 8), (9, 8), (15, 9), (33, 120), (200, 31))
PYRAMID_SIZES = SIZES + ((65, 33), (200, 120))  # 65 -> 33 -> 17 -> 9 and 33 -> 17 -> 9 -> 5: an odd half at every level


def _parallax_scene():
    """initial_xy chosen from the restatement's own forward result: even features get fx - ix = 120 and fy - iy = 160 exactly
    (parallax 200.0f, kept), odd ones the smallest ix below that for which the f32 parallax exceeds 200 (dropped)."""
    w, h = 200, 120
    big = canvas(5, w, h, 4, 1)
    A, B = view(big, w, h, 0, 0), view(big, w, h, 1.3, -0.8)
    gx, gy = np.meshgrid(np.linspace(70.3, 185.2, 8), np.linspace(22.4, 99.1, 5))
    xy = np.stack([gx.ravel(), gy.ravel()], 1).astype(F)
    fwd = R.track_features(A, B, xy, xy)[3]["fwd"]
    init = np.stack([fwd[:, 0] - F(120), fwd[:, 1] - F(160)], 1).astype(F)
    for i in range(1, len(xy), 2):
        while True:
            init[i, 0] = np.nextafter(init[i, 0], F(-np.inf))
            dx, dy = fwd[i, 0] - init[i, 0], fwd[i, 1] - init[i, 1]
            if np.sqrt(dx * dx + dy * dy) > F(200):
                break
    return scene(A, B, xy, init)


@functools.lru_cache(maxsize=None)
def scenes():
    S = {}
    S["size_8x8"] = size_scene(8, 8, (0.4, -0.3), 7, 7)
    S["size_9x8"] = size_scene(9, 8, (0.5, 0.2), 7, 7)
    S["size_15x9"] = size_scene(15, 9, (-0.6, 0.3), 8, 7)
    S["size_33x120"] = size_scene(33, 120, (0.3, -7.2), 7, 14, [tile_edge_points(33, 120)])
    S["size_200x31"] = size_scene(200, 31, (6.5, 0.4), 16, 7, [tile_edge_points(200, 31)])
    big = canvas(3, 96, 64, 3, 1)
    A, B = view(big, 96, 64, 0, 0), view(big, 96, 64, 0.7, 0.4)
    A[:, 48:] = 90
    B[:, 48:] = 90
    S["flat_half"] = scene(A, B, grid(96, 64, 10, 6, out=4.0))
    A, B = nyquist_pair(64, 48)
    S["nyquist"] = scene(A, B, grid(64, 48, 7, 5, out=-6.0))
    for k, sh in enumerate(((56.0, 40.0), (-56.0, -40.0), (48.0, -44.0), (-52.0, 46.0))):
        S["far_%d" % k] = shifted(40 + k, 200, 120, sh, grid(200, 120, 9, 6, out=-4.0), cell=10, smooth=4)
    S["rough"] = shifted(50, 200, 120, (3.0, -2.0), grid(200, 120, 12, 8, out=2.0), cell=1, smooth=0)
    e = np.arange(0.05, 0.65, 0.05)
    walk = [(110 - d, 40.3) for d in e] + [(60.3, 90 - d) for d in e] + [(-11 + d, 40.3) for d in e] + [(60.3, -11 + d) for d in e]
    big = canvas(6, 100, 80, 3, 1)
    S["edge_walk_out"] = scene(view(big, 100, 80, 0, 0), view(big, 100, 80, 0.3, 0.3), walk)
    S["edge_walk_in"] = scene(view(big, 100, 80, 0, 0), view(big, 100, 80, -0.3, -0.3), walk)
    fr = [0.0, 0.5, 2.0 ** -15, 3 * 2.0 ** -15, 5 * 2.0 ** -15]
    ties = [(30 + 7 * i + fa, 24 + 5 * j + fb) for i, fa in enumerate(fr) for j, fb in enumerate(fr) if (fa not in (0.0, 0.5)) != (fb not in (0.0, 0.5))]
    big = canvas(7, 100, 80, 3, 1)
    S["ties"] = scene(view(big, 100, 80, 0, 0), view(big, 100, 80, 0.6, -0.4), ties)
    A, B = blocks_pair(96, 72)
    S["blocks"] = scene(A, B, grid(96, 72, 8, 6, out=-12.0))
    for name, (seed, sh, cell, smooth, p) in FINAL_OUT.items():
        big = canvas(seed, 100, 80, cell, smooth)
        near = [(p[0] + dx, p[1] + dy) for dx in (-0.5, 0.0, 0.5) for dy in (-0.5, 0.0, 0.5)]
        S[name] = scene(view(big, 100, 80, 0, 0), view(big, 100, 80, *sh), [p] + near)
    for name, (seed, sh, p) in BAND.items():
        big = canvas(seed, 72, 56, 3, 1)
        S[name] = scene(view(big, 72, 56, 0, 0), view(big, 72, 56, *sh), [p, (p[0] + 3.0, p[1]), (p[0], p[1] + 3.0)])
    A, B = fb_exact_pair()
    S["fb_exactly_2"] = scene(A, B, [(32, 24), (32, 16), (32, 32), (32, 20), (31, 24)])
    S["parallax_200"] = _parallax_scene()
    S["empty"] = scene(S["ties"]["A"], S["ties"]["B"], np.zeros((0, 2), F))
    for n in COUNTS:
        S["count_%d" % n] = count_scene(n)
    for s in S.values():  # built once, shared by every test
        for k in ("A", "B", "xy", "init"):
            s[k].setflags(write=False)
    return S


SCENE_NAMES = ("size_8x8", "size_9x8", "size_15x9", "size_33x120", "size_200x31", "flat_half", "nyquist", "far_0", "far_1", "far_2",
               "far_3", "rough", "edge_walk_out", "edge_walk_in", "ties", "blocks") + tuple(FINAL_OUT) + tuple(BAND) + ("fb_exactly_2", "parallax_200", "empty") + tuple("count_%d" % n for n in COUNTS)


@functools.lru_cache(maxsize=None)
def ref(name, mutation=None):
    """The restatement's answer on a scene, computed once and shared (read-only): kept_xy, kept_index, av_parallax, counters
    (which hold the forward pass, `fwd` and `status1`: what lk_track returns)."""
    s = scenes()[name]
    kxy, kidx, av, rec = R.track_features(s["A"], s["B"], s["xy"], s["init"], mutation=mutation)
    for a in (kxy, kidx, rec["fwd"], rec["status1"]):
        a.setflags(write=False)
    return kxy, kidx, av, rec


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _same_track(got, want):
    """(kept_xy, kept_index, av_parallax) against the restatement's: indices, f32 position bits, av_parallax bits."""
    return (np.array_equal(got[1], want[1]) and np.array_equal(_bits(got[0]), _bits(want[0]))
            and F(got[2]).view(np.uint32) == F(want[2]).view(np.uint32))


def _same_lk(got, rec):
    return np.array_equal(got[1], rec["status1"]) and np.array_equal(_bits(got[0]), _bits(rec["fwd"]))


def pyramid_image(w, h):
    rng = np.random.default_rng(w * 1000 + h)
    img = rng.integers(0, 256, (h, w), dtype=np.uint8)
    img[::7, ::5] = 255
    img[3::11, 1::9] = 0
    return img


@functools.lru_cache(maxsize=None)
def ref_pyramid(w, h):
    out = R.build_pyramid(pyramid_image(w, h))
    for a in out:
        a.setflags(write=False)
    return out


# -------------------------------------------------------------------------------------------------------------- CPU tests
def test_scene_list_is_complete_and_small():
    S = scenes()
    assert tuple(S) == SCENE_NAMES
    assert max(s["A"].size for s in S.values()) <= 200 * 120
    assert max(len(s["xy"]) for name, s in S.items() if not name.startswith("count_")) <= 200
    assert [ref_pyramid(65, 33)[l].shape for l in range(4)] == [(33, 65), (17, 33), (9, 17), (5, 9)]
    assert [ref_pyramid(8, 8)[l].shape for l in range(4)] == [(8, 8), (4, 4), (2, 2), (1, 1)]


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_oracle_returns_the_restatements_bytes(name):
    import oracle_lib as O
    s = scenes()[name]
    want = ref(name)
    assert _same_lk(O.lk_track(s["A"], s["B"], s["xy"]), want[3])
    got = O.track_features(s["A"], s["B"], s["xy"], s["init"])
    assert _same_track(got, want), (got[2], want[2], len(got[1]), len(want[1]))


@pytest.mark.parametrize("w,h", PYRAMID_SIZES)
def test_oracle_pyramid_equals_the_restatements(w, h):
    import oracle_lib as O
    got = O.build_pyramid(pyramid_image(w, h))
    assert [a.shape for a in got] == [a.shape for a in ref_pyramid(w, h)]
    assert all(np.array_equal(a, b) for a, b in zip(got, ref_pyramid(w, h)))


def test_lk_track_of_the_restatement_is_its_forward_pass():
    for name in ("size_15x9", "ties"):
        s = scenes()[name]
        out, st, rec = R.lk_track(s["A"], s["B"], s["xy"])
        assert _same_lk((out, st), ref(name)[3])
        assert rec["status1_0"] == 0 and rec["tmpl_in"] > 0  # the forward pass alone: nothing of the filter is counted


# What each scene is for: counters of the restatement, exact (forward and backward pass together).
EXPECT = {
    "size_8x8": {"tmpl_out_coarse": 98, "tmpl_out_l0": 122, "eig_low_l3": 162, "eig_low_l12": 268, "eig_low_l0": 25, "eig_ok": 29, "exit_eps": 27, "exit_osc": 2},
    "size_9x8": {"tmpl_out_coarse": 94, "tmpl_out_l0": 122, "eig_low_l3": 162, "eig_low_l12": 267, "eig_low_l0": 20, "eig_ok": 39, "exit_eps": 39, "exit_osc": 0},
    "size_15x9": {"tmpl_out_coarse": 94, "tmpl_out_l0": 132, "eig_low_l3": 176, "eig_low_l12": 245, "eig_low_l0": 25, "eig_ok": 88, "exit_eps": 56, "exit_osc": 32},
    "size_33x120": {"tmpl_out_coarse": 128, "tmpl_out_l0": 125, "eig_low_l0": 66, "iter_out_coarse": 9, "iter_out_l0": 7, "exit_cap": 2, "tile_x_end_at_w": 1,
                    "tile_x_end_w_minus_1": 1, "tile_x_end_w_plus_1": 1, "tile_y_end_at_h": 1, "tile_y_end_h_minus_1": 1, "tile_y_end_h_plus_1": 1, "fb_fail": 2},
    "size_200x31": {"tmpl_out_coarse": 133, "tmpl_out_l0": 137, "eig_low_l0": 64, "iter_out_coarse": 5, "iter_out_l0": 6, "exit_cap": 1, "tile_x_end_at_w": 1,
                    "tile_x_end_w_minus_1": 1, "tile_x_end_w_plus_1": 1, "tile_y_end_at_h": 2, "tile_y_end_h_minus_1": 1, "tile_y_end_h_plus_1": 2, "fb_fail": 0},
    "flat_half": {"eig_low_l0": 51, "eig_ok": 229, "status1_0": 25},
    "nyquist": {"eig_low_l3": 70, "eig_low_l12": 140, "eig_low_l0": 64, "tracked_l0_after_l3_skip": 6, "status1_after_coarse_skip": 6, "exit_cap": 5},
    "far_0": {"iter_out_coarse": 32, "iter_out_l0": 33, "exit_cap": 138, "stage_restage": 151, "stage_xpos": 31, "stage_xneg": 27, "stage_ypos": 57, "stage_yneg": 41,
              "stage_in_to_reflect": 3, "stage_reflect_to_in": 4, "fb_fail": 18},
    "far_1": {"iter_out_coarse": 33, "iter_out_l0": 24, "exit_cap": 119, "stage_restage": 125, "stage_xpos": 35, "stage_xneg": 24, "stage_ypos": 49, "stage_yneg": 22,
              "stage_in_to_reflect": 6, "stage_reflect_to_in": 5, "fb_fail": 24},
    "far_2": {"iter_out_coarse": 11, "iter_out_l0": 21, "exit_cap": 120, "stage_restage": 90, "stage_xpos": 29, "stage_xneg": 23, "stage_ypos": 21, "stage_yneg": 19,
              "stage_in_to_reflect": 8, "stage_reflect_to_in": 2, "fb_fail": 26},
    "far_3": {"iter_out_coarse": 40, "iter_out_l0": 27, "exit_cap": 164, "stage_restage": 126, "stage_xpos": 32, "stage_xneg": 29, "stage_ypos": 30, "stage_yneg": 39,
              "stage_in_to_reflect": 4, "stage_reflect_to_in": 5, "fb_fail": 22},
    "rough": {"exit_eps": 83, "exit_osc": 354, "exit_cap": 22, "osc_near_below": 34, "osc_near_above": 21},
    "edge_walk_out": {"tmpl_out_l0": 14, "eig_low_l0": 82, "eig_ok": 192},  # templates half a window outside: every derivative under
    "edge_walk_in": {"tmpl_out_l0": 10, "eig_low_l0": 86, "eig_ok": 192},   # them is 0 at level 0, the coarse levels still track
    "ties": {"weight_tie_l0_tmpl": 12, "weight_tie": 12},
    "blocks": {"A_over_2p31": 94, "A_over_2p32": 10, "b_over_2p31": 180, "b_over_2p32_pos": 4, "b_over_2p32_neg": 1, "max_abs_sum": 5179713580,
               "max_abs_3rows": 814299772, "exit_cap": 11},
    "final_out_cap_left": {"final_out": 2, "final_ok": 8, "iter_out_l0": 3, "exit_eps": 17, "exit_osc": 0, "exit_cap": 11},
    "final_out_cap_bottom": {"final_out": 2, "final_ok": 4, "iter_out_l0": 4, "exit_eps": 56, "exit_osc": 4, "exit_cap": 6},
    "final_out_right": {"final_out": 2, "final_ok": 5, "iter_out_l0": 4, "exit_eps": 46, "exit_osc": 19, "exit_cap": 2},
    "final_out_cap_right": {"final_out": 3, "final_ok": 9, "iter_out_l0": 2, "exit_eps": 14, "exit_osc": 0, "exit_cap": 18},
    "band_stop_a": {"band_stop": 1, "band_go": 0},
    "band_stop_b": {"band_stop": 1, "band_go": 0},
    "band_go_a": {"band_stop": 0, "band_go": 1},
    "band_go_b": {"band_stop": 0, "band_go": 1},
    "fb_exactly_2": {"fb_is_2": 4, "fb_fail": 4, "fb_ok": 1, "eig_low_l3": 10, "eig_low_l12": 20, "exit_eps": 9},
    "parallax_200": {"parallax_is_200": 20, "parallax_keep": 20, "parallax_drop": 20, "fb_ok": 40},
    "empty": {"tmpl_in": 0, "status1_0": 0},
    "count_1": {"status1_0": 0, "fb_ok": 1, "parallax_keep": 1},
    "count_63": {"status1_0": 60, "fb_ok": 3, "parallax_keep": 3},
    "count_64": {"status1_0": 61, "fb_ok": 3, "parallax_keep": 3},
    "count_65": {"status1_0": 62, "fb_ok": 3, "parallax_keep": 3},
    "count_1023": {"status1_0": 994, "fb_ok": 29, "parallax_keep": 29},
    "count_1024": {"status1_0": 995, "fb_ok": 29, "parallax_keep": 29},
    "count_1025": {"status1_0": 996, "fb_ok": 29, "parallax_keep": 29},
    "count_4096": {"status1_0": 3984, "fb_ok": 112, "parallax_keep": 112},
    "count_4097": {"status1_0": 3985, "fb_ok": 112, "parallax_keep": 112},
    "count_8200": {"status1_0": 7977, "fb_ok": 223, "parallax_keep": 223},
}
# Counters that no input of the declared domain can move, with the reason; they are asserted to BE zero.
#   det_small_alone             minEig >= 0.01 means lambda_min >= 8.82, so det >= 77; A11, A22 <= 441 * 4080^2 * 2^-20 < 7001 keep the f32
#                               error of A11 A22 - A12^2 below 2^-23 * 7001^2 < 6: D < FLT_EPSILON never decides alone.
#   status1_after_coarse_break  a window that leaves level l at position n (n >= w_l or n < -21) starts the next level at 2 n + 10,
#                               which is outside that level as well (w_(l-1) <= 2 w_l), down to level 0, where the first test of the
#                               loop clears the status: the break keeps the status at ITS level (iter_out_coarse counts it), the
#                               point is lost all the same.
# For the same reason a template window is never outside a coarse level ONLY: -11 <= x < w + 10 at level 0 implies the same test
# at every coarser level (x / 2^l - 10 < w / 2^l), so tmpl_out_coarse is always followed by tmpl_out_l0.
IMPOSSIBLE = ("det_small_alone", "status1_after_coarse_break")
NOT_REACHED = ()  # of the f64 band (band_stop, band_go): both outcomes were found by the bounded search (BAND)


def test_every_scene_reaches_what_it_was_built_for():
    got = {name: {key: int(ref(name)[3][key]) for key in want} for name, want in EXPECT.items()}
    assert got == EXPECT
    assert set(EXPECT) == set(SCENE_NAMES)


def test_every_decision_is_reached_on_some_scene():
    total = {key: sum(int(ref(name)[3][key]) for name in SCENE_NAMES) for key in R.COUNTERS}
    assert set(NOT_REACHED) <= {"band_stop", "band_go"}
    assert tuple(sorted(k for k, v in total.items() if v == 0)) == tuple(sorted(IMPOSSIBLE + NOT_REACHED)), total
    # the skip of a coarse level and the break at one keep the status there; the former is seen in the output
    assert total["status1_after_coarse_skip"] > 0 and total["iter_out_coarse"] > 0 and total["tmpl_out_coarse"] > 0
    for name in SCENE_NAMES:  # a template outside a coarse level is outside level 0 too
        rec = ref(name)[3]
        assert rec["tmpl_out_coarse"] <= 3 * rec["tmpl_out_l0"]


HALF_ROW_BOUND = 7 * 8 * 33292800  # what eight lanes of seven products can reach: the kernel's int32 half-row sum


def test_largest_sums():
    """The blocks scene carries A and b sums beyond 2^32 (b of both signs: the 16-bit split of a negative total), and its
    largest partial over three window rows (63 products, more than the 56 of a half row) is what DESIGN.md records."""
    rec = ref("blocks")[3]
    assert rec["max_abs_sum"] == 5179713580 > 1 << 32 and rec["A_over_2p32"] > 0 and rec["b_over_2p32_pos"] > 0 and rec["b_over_2p32_neg"] > 0
    assert rec["max_abs_3rows"] == 814299772 < HALF_ROW_BOUND
    others = max(int(ref(name)[3]["max_abs_sum"]) for name in SCENE_NAMES if name != "blocks")
    assert others < 1 << 31  # no other scene leaves int32: the wrap mutation shows on `blocks` alone


def test_parallax_threshold_features():
    """Even features: fx - ix = 120 and fy - iy = 160 exactly in f32, parallax 200.0f, kept (the test is >).  Odd features: one
    ulp above 200, dropped."""
    s = scenes()["parallax_200"]
    kxy, kidx, av, rec = ref("parallax_200")
    fwd, init = rec["fwd"], s["init"]
    par = dict(rec["parallax"])
    assert len(par) == len(s["xy"]) == 40
    for i in range(40):
        dx, dy = fwd[i, 0] - init[i, 0], fwd[i, 1] - init[i, 1]
        if i % 2 == 0:
            assert dx == F(120) and dy == F(160) and par[i] == F(200)
        else:
            assert dy == F(160) and par[i] == np.nextafter(F(200), F(np.inf))
    assert kidx.tolist() == list(range(0, 40, 2))
    assert av == F(100.0)  # 20 x 200 / 40: the divisor is the count of ALL features
    assert ref("empty")[2] == F(0) and len(ref("empty")[1]) == 0


# mutation -> the scene named for it (and what the scene holds for it)
MUTATION_SCENE = {
    "round_half_away": "ties",              # weights x.5 with x even at level 0
    "wrap_int32": "blocks",                 # sums beyond 2^32
    "parallax_ge": "parallax_200",          # parallax == 200.0f
    "fb_le": "fb_exactly_2",                # forward-backward distance exactly 2.0
    "deriv_reflect": "size_33x120",         # windows over the border
    "border_replicate": "size_8x8",         # levels 1 to 4 px wide
    "no_half_step": "rough",                # 354 oscillation exits
    "skip_sets_status": "nyquist",          # levels 1 to 3 flat, level 0 tracked
    "mean_over_kept": "count_63",           # 3 kept of 63
    "pairwise_sum": "count_4097",           # 112 kept parallaxes whose two sums differ in the last place
    "no_final_check": "final_out_right",    # a last step that leaves the image
}


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_every_misreading_changes_its_scenes_bytes(mutation):
    import oracle_lib as O
    assert tuple(MUTATION_SCENE) == R.MUTATIONS
    name = MUTATION_SCENE[mutation]
    s = scenes()[name]
    mut = ref(name, mutation)
    assert not (_same_track(mut[:3], ref(name)) and _same_lk((mut[3]["fwd"], mut[3]["status1"]), ref(name)[3]))
    oracle = O.track_features(s["A"], s["B"], s["xy"], s["init"])
    assert not (_same_track(oracle, mut) and _same_lk(O.lk_track(s["A"], s["B"], s["xy"]), mut[3]))


# -------------------------------------------------------------------------------------------------------------- GPU tests
GPU_SCENES = tuple(name for name in SCENE_NAMES if not name.startswith("count_"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", GPU_SCENES)
def test_hip_returns_the_restatements_bytes(ctx, name):
    """svo_lk_track and svo_track_features against the restatement (not the oracle): status, f32 position bits, kept indices
    and the bits of av_parallax."""
    s = scenes()[name]
    want = ref(name)
    assert _same_lk(ctx.lk_track(s["A"], s["B"], s["xy"]), want[3])
    got = ctx.track_features(s["A"], s["B"], s["xy"], s["init"])
    assert _same_track(got, want), (got[2], want[2], len(got[1]), len(want[1]))


@pytest.mark.gpu
def test_hip_feature_counts_around_the_compaction_blocks():
    """1 to 8200 features in a context of its own (the session's is created for 4096): the 64-lane ballots, the 1024-thread
    rounds and, beyond 4096, the restaged parallax sum of track_compact_kernel.  Then small calls again on the same context."""
    import stereo_vo_amd as S
    c = S.Context(256, 128, max_batch=1, max_corners=256, max_candidates=1 << 12, max_features=8320)
    try:
        for n in COUNTS + (4097, 1, 65):
            s = scenes()["count_%d" % n]
            want = ref("count_%d" % n)
            got = c.track_features(s["A"], s["B"], s["xy"], s["init"])
            assert _same_track(got, want), (n, got[2], want[2], len(got[1]), len(want[1]))
            assert _same_lk(c.lk_track(s["A"], s["B"], s["xy"]), want[3]), n
    finally:
        c.close()


@pytest.mark.gpu
def test_hip_result_does_not_depend_on_the_calls_before_it(ctx):
    """One context reuses its workspace: a long call, an empty one, a small image, the largest sums, and the first again."""
    for name in ("far_0", "empty", "size_8x8", "blocks", "count_4097", "parallax_200", "far_0"):
        s = scenes()[name]
        assert _same_track(ctx.track_features(s["A"], s["B"], s["xy"], s["init"]), ref(name)), name


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", PYRAMID_SIZES)
def test_hip_pyramid_equals_the_restatements(ctx, w, h):
    got = ctx.build_pyramid(pyramid_image(w, h))
    assert [a.shape for a in got] == [a.shape for a in ref_pyramid(w, h)]
    assert all(np.array_equal(a, b) for a, b in zip(got, ref_pyramid(w, h)))


@pytest.mark.gpu
def test_hip_per_level_pyramid_equals_the_restatements():
    """SVO_PYR_PER_LEVEL=1 (pyr_down_kernel per level instead of pyr_build_kernel) is read once per process: a child process
    builds every size and writes the levels; they are compared here."""
    here = os.path.dirname(os.path.abspath(__file__))
    with tempfile.TemporaryDirectory() as tmp:
        src, dst = os.path.join(tmp, "in.npz"), os.path.join(tmp, "out.npz")
        np.savez(src, **{"%dx%d" % (w, h): pyramid_image(w, h) for w, h in PYRAMID_SIZES})
        env = dict(os.environ, SVO_PYR_PER_LEVEL="1")
        r = subprocess.run([sys.executable, os.path.join(here, "_lk_pyr_per_level_worker.py"), src, dst], env=env, capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        out = np.load(dst)
        for w, h in PYRAMID_SIZES:
            for l, want in enumerate(ref_pyramid(w, h)):
                assert np.array_equal(out["%dx%d_%d" % (w, h, l)], want), (w, h, l)
