"""The code that joins the stages -- ImageProcessor::process, the FeatureTracker state, the BundleAdjuster graph edits, the window
gather and write-back, the driver rule -- on streams that reach every decision, judged by an independent restatement
(tests/pipeline_ref.py, written from the reference source; the window solve is the oracle's ba_solve, pinned to ba_ref in
tests/test_ba_ref.py).

`tests/test_pipeline.py` and `tests/test_group.py` compare the three implementations of one hand (oracle/ora_pipeline.cpp,
host/pipeline.cpp, host/group.cpp) with each other on mild synthetic drives.  Here the oracle (CPU), svo_pipeline_* and
svo_pipeline_group_* (GPU; the only way to lk_fb_group_kernel and pnp_group_kernel) must return the restatement's bytes after every
frame: the six counts, av_parallax and percent_lost as bit patterns (NaN included), the float pose with ==, the tracked ids and
positions.  No tolerance anywhere except the ba_ref-derived one of the CPU cost check.

The streams are 248 x 96 views of block-noise canvases (tests/test_lk_paths.py canvas), the right image the left view 8 px
further: a fronto-parallel plane, so an image shift is a sideways step and an in-plane rotation a roll.  StereoBM(48, 21), 80 corners.
Frames, keyframes and the counters of pipeline_ref each case turns (measured by the run that wrote this table):

base-plain     10 frames  5 keyframes  gate_parallax_alone=4 gate_not_taken=5 window_popped=2 popped_landmark_still_observed=94 quat_trace_pos=4
base-blank      9 frames  4 keyframes  skip_before_first=1 skip_after_first=2 gate_parallax_alone=3 gate_not_taken=2 window_popped=1
base-cut        9 frames  5 keyframes  gate_parallax_alone=3 gate_loss_alone=1 gate_not_taken=4 pnp_no_model=1 window_popped=2
base-nodisp1    6 frames  4 keyframes  gate_loss_alone=1 percent_lost_nan=1 pnp_m0=1 pnp_no_model=1 window_popped=1 rodrigues_small=1
base-nodisp6    9 frames  8 keyframes  gate_loss_alone=6 percent_lost_nan=6 pnp_m0=6 pnp_no_model=6 window_popped=5 rodrigues_small=6
base-occlude    6 frames  3 keyframes  gate_loss_alone=1 gate_both=1 gate_not_taken=3
base-roll      13 frames 13 keyframes  gate_parallax_alone=12 inliers_lt_tracked=3 window_popped=10 quat_trace_pos=11 quat_z=1
base-island     4 frames  2 keyframes  gate_parallax_alone=1 gate_not_taken=2 dedup_dropped_all=1
base-sheet      5 frames  3 keyframes  gate_loss_alone=2 gate_not_taken=2 inliers_lt_tracked=1 dedup_dropped_none=1
mf50-*         plain / cut / blank with max_features 50: new_truncated=3 / 2 / 3, max_new_zero=1 each
mf20-*         the same with max_features 20: new_truncated=5 / 5 / 4, max_new_zero=3 / 3 / 2
win1-*         the same with window_size 1: window_popped=4 / 4 / 3, popped_landmark_still_observed=206 / 141 / 166
every-*        the same with parallax_thresh -1 (a keyframe on every frame that is not skipped): 10 / 9 / 6 keyframes, gate_both=1 (cut)
n64-drift       4 frames  2 keyframes  64 features into the tracker (max_features 64), PnP on 64: one round of the grouped compaction
n65-drift       4 frames  2 keyframes  117 features into the tracker, PnP on 117: two rounds

Never turned, and why (pipeline_ref.UNREACHABLE): the C-5 guard cannot fire from process() (num_tracked <= max_features by induction),
the x and y sub-cases of the quaternion fall-back need a camera rolled about an image axis (tests/sanitize/det_trig_test.cpp runs them).
One listed misreading, `<=` for the loss test, is an equivalent mutant (test_loss_le_cannot_differ).

Wall time, measured: the CPU part 44 s (23 reference runs of 0.4 to 4 s each, cached for the session, the oracle on each, 10 mutations,
the cost check); the GPU part 13 s for 60 tests on an MI355X, the cached references included (the roll stream's 1.5 s is the longest).
"""
import functools

import numpy as np
import pytest

import pipeline_ref as PR

F = np.float32
gpu = pytest.mark.gpu
W, H, MARGIN = 248, 96, 104
DISPARITY = 8.0
BLANK = np.full((H, W), 90, np.uint8)

# the camera: a fronto-parallel plane at focal * baseline / DISPARITY = 18.75 m; a shift of the image is a sideways step of the
# camera and an in-plane rotation about (cx, cy) a roll, so every stream is a rigid motion that PnP can explain
BASE = dict(focal=300.0, cx=124.0, cy=48.0, baseline=0.5, width=W, height=H, max_corners=80, quality=0.1, min_feature_distance=10.0,
            parallax_thresh=6.0, window_size=3, max_features=400)
PARAMS = {
    "base": BASE,
    "mf50": dict(BASE, max_features=50),
    "mf20": dict(BASE, max_features=20),
    "win1": dict(BASE, window_size=1),
    "every": dict(BASE, parallax_thresh=-1.0),
    "n64": dict(BASE, max_corners=200, min_feature_distance=6.0, max_features=64),
    "n65": dict(BASE, max_corners=200, min_feature_distance=6.0),
}


# ---------------------------------------------------------------------------------------------------------------- streams
@functools.lru_cache(maxsize=None)
def canvas(seed, cell=3, smooth=1):
    from test_lk_paths import canvas as lk_canvas
    return lk_canvas(seed, W, H, cell, smooth, margin=MARGIN)


def render(big, angle=0.0, shift=(0.0, 0.0), disparity=0.0):
    """The W x H view of the canvas rotated by `angle` about the image centre and displaced by `shift`, bilinear, rounded to uint8; with
    `disparity` d the view whose pixel (x, y) shows what the left view shows at (x + d, y): the right image of a plane at one depth."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    u, v = xx + disparity - (W - 1) / 2 - shift[0], yy - (H - 1) / 2 - shift[1]
    c, s = np.cos(angle), np.sin(angle)
    x = c * u + s * v + (W - 1) / 2 + MARGIN
    y = -s * u + c * v + (H - 1) / 2 + MARGIN
    x0, y0 = np.floor(x).astype(int), np.floor(y).astype(int)
    assert x0.min() >= 0 and y0.min() >= 0 and x0.max() + 1 < big.shape[1] and y0.max() + 1 < big.shape[0]
    fx, fy = x - x0, y - y0
    val = (big[y0, x0] * (1 - fx) * (1 - fy) + big[y0, x0 + 1] * fx * (1 - fy) + big[y0 + 1, x0] * (1 - fx) * fy +
           big[y0 + 1, x0 + 1] * fx * fy)
    return np.clip(np.rint(val), 0, 255).astype(np.uint8)


def pair(big, angle=0.0, shift=(0.0, 0.0)):
    return render(big, angle, shift), render(big, angle, shift, DISPARITY)


def drive(seed, n, step=(3.3, 0.9)):
    big = canvas(seed)
    return [pair(big, 0.0, (step[0] * k, step[1] * k)) for k in range(n)]


def stream_plain():
    return drive(11, 10)


def stream_blank():
    """Blank at frame 0 (skipped before the first keyframe) and at frames 4 and 5 (skipped after it: the tracker keeps frame 3)."""
    fr = drive(12, 9)
    for k in (0, 4, 5):
        fr[k] = (BLANK, BLANK)
    return fr


def stream_cut():
    """Another scene from frame 5 on: nothing of the old one is found again."""
    return drive(13, 5) + drive(14, 4)


def stream_nodisp1():
    """The first keyframe's right image is flat: no corner has a disparity (tests/test_geom_paths.py::test_hip_keyframe_without_any_disparity)."""
    fr = drive(15, 6)
    fr[0] = (fr[0][0], BLANK)
    return fr


def stream_nodisp6():
    fr = drive(16, 9)
    for k in range(6):
        fr[k] = (fr[k][0], BLANK)
    return fr


def stream_occlude():
    """A flat sheet slides in from the left over a drive that is slow at first.  Frame 2: the sheet covers x < 160, more than 0.4 of the
    features are lost while the others have hardly moved (the loss side of the gate fires alone).  Frame 3 steps 5.8 px (below the
    threshold), frame 4 another 8 px while the sheet grows to x < 213: 0.45 of the features are lost and the mean over ALL of them
    (SURVEY C-2) is still above the threshold (both sides fire)."""
    big = canvas(17)
    shift = (0.0, 0.4, 0.8, 6.6, 14.6, 15.6)
    edge = (0, 0, 160, 160, 213, 213)
    out = []
    for s, e in zip(shift, edge):
        L, R = pair(big, 0.0, (s, 0.1 * s))
        L, R = L.copy(), R.copy()
        L[:, :e] = 90
        R[:, :max(e - int(DISPARITY), 0)] = 90
        out.append((L, R))
    return out


ROLL_STEP, ROLL_FRAMES = 0.19, 13


def stream_roll():
    """In-plane rotation by ROLL_STEP rad per frame: the accumulated rvec passes 120 degrees (trace(R) <= 0) before the stream ends."""
    big = canvas(18)
    return [pair(big, ROLL_STEP * k) for k in range(ROLL_FRAMES)]


def stream_drift():
    """A slow drive for the feature-count cases: nothing is lost in frame 1, every parallax is a different non-zero number, and frame 3 is
    a keyframe: PnP on every tracked feature."""
    return drive(19, 4, step=(2.2, 0.5))


def stream_island():
    """Texture only on an island well inside StereoBM's valid rectangle: every corner gets a disparity and is tracked, so at the next
    keyframe every detected corner is the duplicate of an inlier."""
    big = np.full_like(canvas(20), 128.0)
    big[MARGIN + 18:MARGIN + 76, MARGIN + 84:MARGIN + 200] = canvas(20)[MARGIN + 18:MARGIN + 76, MARGIN + 84:MARGIN + 200]
    return [pair(big, 0.0, (3.3 * k, 0.9 * k)) for k in range(4)]


def stream_sheet():
    """A low-contrast scene driven fast.  From frame 2 on a full-contrast sheet, fixed in the image, covers the left part: its corners are
    16 times stronger than the scene's, so every detected corner lies on the sheet, more than min_feature_distance from each of the few
    inliers on the right (the dedup drops none), and PnP finds fewer inliers than features."""
    big = 128.0 + (canvas(21) - 128.0) * 0.25
    rng = np.random.default_rng(22)
    sheet = np.kron(rng.integers(0, 2, (H // 6 + 1, 20)) * 255, np.ones((6, 6)))[:H, :]
    out = []
    for k in range(5):
        L, R = pair(big, 0.0, (14.0 * k, 1.0 * k))
        if k >= 2:
            L, R = L.copy(), R.copy()
            d = int(DISPARITY)
            L[:, 40:125], L[:, 125:142] = sheet[:, 0:85], 128
            R[:, 40 - d:125 - d], R[:, 125 - d:142 - d] = sheet[:, 0:85], 128
        out.append((L, R))
    return out


STREAMS = {"plain": stream_plain, "blank": stream_blank, "cut": stream_cut, "nodisp1": stream_nodisp1, "nodisp6": stream_nodisp6,
           "occlude": stream_occlude, "roll": stream_roll, "drift": stream_drift, "island": stream_island, "sheet": stream_sheet}
BASE_STREAMS = ("plain", "blank", "cut", "nodisp1", "nodisp6", "occlude", "roll", "island", "sheet")
MIXED = ("plain", "cut", "blank")
CASES = [("base", s) for s in BASE_STREAMS] + [(p, s) for p in ("mf50", "mf20", "win1", "every") for s in MIXED] + \
        [("n64", "drift"), ("n65", "drift")]


@functools.lru_cache(maxsize=None)
def frames(name):
    return STREAMS[name]()


# -------------------------------------------------------------------------------------------------------------- references
# which counters each stream is built to turn (asserted per stream on the CPU); together they are every reachable counter
TURNS = {
    ("base", "plain"): ("gate_parallax_alone", "gate_not_taken", "window_popped", "popped_landmark_still_observed", "quat_trace_pos"),
    ("base", "blank"): ("skip_before_first", "skip_after_first"),
    ("base", "cut"): ("gate_loss_alone", "pnp_no_model"),
    ("base", "nodisp1"): ("percent_lost_nan", "pnp_m0", "pnp_no_model", "rodrigues_small"),
    ("base", "nodisp6"): ("percent_lost_nan", "pnp_m0", "rodrigues_small", "window_popped"),
    ("base", "occlude"): ("gate_loss_alone", "gate_both"),
    ("base", "roll"): ("quat_z", "quat_trace_pos", "inliers_lt_tracked"),
    ("base", "island"): ("dedup_dropped_all",),
    ("base", "sheet"): ("dedup_dropped_none", "inliers_lt_tracked"),
    ("mf50", "plain"): ("new_truncated", "max_new_zero"),
    ("mf20", "plain"): ("new_truncated", "max_new_zero"),
    ("win1", "plain"): ("window_popped", "popped_landmark_still_observed"),
    ("every", "cut"): ("gate_both",),
}
# the stream that tells each misreading from the reference
CAUGHT_BY = {"gate_or": ("base", "nodisp1"), "lost_vs_previous": ("base", "sheet"), "all_tracked_into_keyframe": ("base", "sheet"),
             "dedup_all_tracked": ("base", "sheet"), "truncate_before_tracked": ("mf20", "plain"), "ids_reused": ("win1", "plain"),
             "pop_late": ("base", "nodisp1"), "hmat_no_transpose": ("base", "sheet"), "initial_not_reset": ("base", "island"),
             "gather_pose_major": ("base", "island")}


def key(r):
    """The six counts, av_parallax and percent_lost as bit patterns (NaN included), pose7 with ==."""
    return (r.n_detected, r.n_tracked, r.n_inliers, r.n_new, r.is_keyframe, r.ba_iterations,
            int(F(r.av_parallax).view(np.uint32)), int(F(r.percent_lost).view(np.uint32)), tuple(float(v) for v in r.pose7))


def tracked_bytes(ids, xy):
    return np.asarray(ids, np.int64).tobytes(), np.ascontiguousarray(xy, F).tobytes()


def run_reference(pname, sname, variant=None):
    """[(key, tracked ids, tracked positions) per frame], the counters, the gathered problems with the solve's summaries."""
    import oracle_lib as O
    p = PARAMS[pname]
    problems, summaries = [], []

    def solve(poses, points, op, oj, uv):
        poses, points, s = O.ba_solve(poses, points, op, oj, uv, p["focal"], p["cx"], p["cy"], max_iterations=50, num_threads=4)
        summaries.append(s)
        return poses, points, s["iterations"]
    ref = PR.Pipeline(solve, variant=variant, problems=problems, **p)
    out = []
    for L, R in frames(sname):
        r = ref.process(L, R)
        out.append((key(r),) + tracked_bytes(*ref.tracked()))
    assert not ref.avail_ids or variant == "ids_reused"  # SURVEY C-3: sequential ids follow from the refcounts as written
    return out, ref.rec, problems, summaries


@functools.lru_cache(maxsize=None)
def reference(pname, sname):
    return run_reference(pname, sname)


# -------------------------------------------------------------------------------------------------------------- CPU tests
@pytest.mark.parametrize("case", sorted(TURNS), ids="-".join)
def test_stream_turns_its_counters(case):
    rec = reference(*case)[1]
    assert all(rec[c] >= 1 for c in TURNS[case]), (case, rec)


def test_streams_together_turn_every_reachable_counter():
    """Every counter of pipeline_ref is named by some stream of TURNS, except those that process() cannot reach (pipeline_ref.UNREACHABLE:
    the C-5 guard, which stays 0 on every stream, and the x / y sub-cases of the quaternion fall-back, which tests/sanitize/det_trig_test.cpp runs)."""
    named = {c for cs in TURNS.values() for c in cs}
    assert named == set(PR.COUNTERS) - set(PR.UNREACHABLE), set(PR.COUNTERS) - named
    for case in CASES:
        assert all(reference(*case)[1][c] == 0 for c in PR.UNREACHABLE), case


@pytest.mark.parametrize("case", CASES, ids="-".join)
def test_oracle_pipeline_returns_the_reference_bytes(case):
    import oracle_lib as O
    ref = reference(*case)[0]
    ora = O.Pipeline(ba_max_iterations=50, num_threads=4, **PARAMS[case[0]])
    for k, (L, R) in enumerate(frames(case[1])):
        r = ora.process(L, R)
        got = (key(r),) + tracked_bytes(*ora.tracked())
        assert got[0] == ref[k][0], (case, k, got[0], ref[k][0])
        assert got[1:] == ref[k][1:], (case, k)


@pytest.mark.parametrize("variant", [v for v in PR.VARIANTS if v not in PR.EQUIVALENT_VARIANTS])
def test_every_mutation_changes_the_bytes_of_its_stream(variant):
    case = CAUGHT_BY[variant]
    out = run_reference(case[0], case[1], variant)[0]
    assert out != reference(*case)[0], (variant, case)


def test_loss_le_cannot_differ():
    """`percent_lost <= 0.4` instead of `< 0.4` is an equivalent mutant: percent_lost is the float of 1.0 - (float) kept / (float) size,
    the comparison is made in double, and no float equals the double 0.4.  Shown for every size up to 4096 and every kept <= size."""
    size = np.arange(1, 4097, dtype=np.float32)[:, None]
    kept = np.arange(0, 4097, dtype=np.float32)[None, :]
    lost = (1.0 - (kept / size).astype(np.float64)).astype(np.float32).astype(np.float64)
    assert not (lost[kept <= size] == 0.4).any()
    assert float(np.float32(0.4)) != 0.4


def test_gathered_window_cost_equals_the_solve_s_initial_cost():
    """At each keyframe of the plain stream: the initial cost of the gathered window problem by ba_ref's residual equals the initial cost
    the solve reports.  Tolerance: ba_ref's own rule as in tests/test_ba_ref.py cost_tolerance, with this camera: 16 x the spread of the
    initial cost among ba_ref's routes, relative, not below COST_FLOOR, and not below the cost of residuals that are all at their floor
    (pose floor x focal length).  That rule was made for residuals of a pixel and for residuals of exactly 0.  Here they are 7e-6 px at
    the first keyframe (the float rounding of the triangulated points) and 0.05 px later, each the difference of two pixel coordinates
    c of up to 250: a residual carries an error of the order of eps x |c|, which moves the cost by |r| times that, more than 1e-14 of a
    cost whose residuals are this small.  The floor therefore also holds this first-order term, sum |r| x 16 eps (|projection| +
    |observation|): MARGIN and the double format's eps, no new constant.  Measured differences: 1.7e-19 at the first keyframe
    (cost 9.6e-10, tolerance 3.1e-16), 7.8e-16 to 2.3e-14 at the later ones (costs 0.08 to 0.8, tolerances 1.9e-12 to 1.1e-11)."""
    import ba_ref as R
    p = PARAMS["base"]
    _, _, problems, summaries = reference("base", "plain")
    assert len(problems) == len(summaries) >= 4
    eps = np.finfo(np.float64).eps
    for prob, s in zip(problems, summaries):
        r = R.residuals(prob["poses0"], prob["points0"], prob["op"], prob["oj"], prob["uv"], p["focal"], p["cx"], p["cy"])
        cost = R.cost_of(r)
        routes = [R.solve(prob, 1, route, rev, p["focal"], p["cx"], p["cy"])[2].initial_cost for route, rev in R.routes_for(prob)]
        spread = (max(routes) - min(routes)) / max(abs(routes[0]), np.finfo(float).tiny)
        size = np.abs(r + prob["uv"]) + np.abs(prob["uv"])
        floor = len(prob["op"]) * (p["focal"] * R.POSE_FLOOR) ** 2 + float((np.abs(r) * R.MARGIN * eps * size).sum())
        tol = max(max(R.MARGIN * spread, R.COST_FLOOR) * abs(cost), floor)
        print("window of %d poses, %d observations: initial cost %.17g, solve %.17g, difference %.3e (tolerance %.3e)" %
              (len(prob["poses0"]), len(prob["op"]), cost, s["initial_cost"], abs(cost - s["initial_cost"]), tol))
        assert abs(cost - s["initial_cost"]) <= tol


# -------------------------------------------------------------------------------------------------------------- GPU tests
def _pipeline_params(S, p):
    pp = S.pipeline_default_params()
    pp.cam.focal, pp.cam.cx, pp.cam.cy, pp.cam.baseline = p["focal"], p["cx"], p["cy"], p["baseline"]
    pp.width, pp.height, pp.max_corners, pp.quality = p["width"], p["height"], p["max_corners"], p["quality"]
    pp.min_feature_distance, pp.parallax_thresh = p["min_feature_distance"], p["parallax_thresh"]
    pp.window_size, pp.max_features, pp.ba_max_iterations = p["window_size"], p["max_features"], 50
    pp.ba_max_time_s = 0.0  # deterministic: iteration cap only (SURVEY C-10)
    return pp


@gpu
@pytest.mark.parametrize("batch", [1, 4])
@pytest.mark.parametrize("case", CASES, ids="-".join)
def test_hip_pipeline_returns_the_reference_bytes(ctx, case, batch):
    """svo_pipeline_process_batch on every stream, in batches of 1 and of 4 frames: every frame's counts, av_parallax and percent_lost
    bits and float pose, and the tracked list after every batch, are the reference's."""
    import stereo_vo_amd as S
    ref = reference(*case)[0]
    fr = frames(case[1])
    g = S.Pipeline(ctx, _pipeline_params(S, PARAMS[case[0]]))
    try:
        for b0 in range(0, len(fr), batch):
            res = g.process_batch(np.stack([f[0] for f in fr[b0:b0 + batch]]), np.stack([f[1] for f in fr[b0:b0 + batch]]))
            for k, r in enumerate(res):
                assert key(r) == ref[b0 + k][0], (case, b0 + k, key(r), ref[b0 + k][0])
            assert tracked_bytes(*g.tracked()) == ref[b0 + len(res) - 1][1:], (case, b0)
    finally:
        g.close()


GROUPS = {pname: [s for q, s in CASES if q == pname] for pname in PARAMS}


@gpu
@pytest.mark.parametrize("batch", [1, 4])
@pytest.mark.parametrize("pname", sorted(GROUPS))
def test_hip_group_lanes_return_their_reference_bytes(pname, batch):
    """The streams that share parameters as the lanes of ONE group: lanes sit in different states in the same launches (one is blank or
    cut, one has no tracked feature at all, one loses half of them while another makes a keyframe).  This is the only way to
    lk_fb_group_kernel and pnp_group_kernel.  A lane whose stream has ended is fed blank frames: they are skipped (SURVEY C-7) and
    leave its tracker as it was.  n64 / n65: 64 and 117 tracked features, one and two rounds of the grouped tracker's compaction."""
    import stereo_vo_amd as S
    names = GROUPS[pname]
    p = PARAMS[pname]
    lanes = len(names)
    refs = [reference(pname, s)[0] for s in names]
    n = max(len(r) for r in refs)
    n = (n + batch - 1) // batch * batch
    Ls = np.stack([np.stack([frames(s)[k][0] if k < len(frames(s)) else BLANK for k in range(n)]) for s in names])
    Rs = np.stack([np.stack([frames(s)[k][1] if k < len(frames(s)) else BLANK for k in range(n)]) for s in names])
    if pname in ("n64", "n65"):
        fed = len(np.frombuffer(refs[0][0][1], np.int64))
        assert fed == 64 if pname == "n64" else fed > 64
    c = S.Context(W, H, max_batch=lanes * batch, max_corners=p["max_corners"], max_candidates=1 << 16, max_features=400)
    try:
        g = S.PipelineGroup(c, _pipeline_params(S, p), lanes)
        try:
            for b0 in range(0, n, batch):
                res = g.process_batch(Ls[:, b0:b0 + batch], Rs[:, b0:b0 + batch])
                for l, ref in enumerate(refs):
                    for k, r in enumerate(res[l]):
                        if b0 + k < len(ref):
                            assert key(r) == ref[b0 + k][0], (names[l], b0 + k, key(r), ref[b0 + k][0])
                        else:
                            assert (r.n_detected, r.n_tracked, r.is_keyframe) == (0, 0, 0) and tuple(r.pose7) == ref[-1][0][8], (names[l], b0 + k)
                    assert tracked_bytes(*g.get_tracked(l)) == ref[min(b0 + batch, len(ref)) - 1][1:], (names[l], b0)
        finally:
            g.close()
    finally:
        c.close()
