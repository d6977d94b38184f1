"""The code that joins the stages, stated once more from the reference's text: ImageProcessor::process
(src/image_processor.cpp:18-163), the FeatureTracker state (src/feature_tracker.cpp:3-72), the BundleAdjuster graph edits,
the window problem and its write-back (src/bundle_adjuster.cpp:41-163) and the driver rule "process(), then bundle_adjust() while
a keyframe exists" (src/vo_node.cpp:141-148).  Plain Python / numpy.  TEST INFRASTRUCTURE ONLY; imports neither the oracle nor
the library, and was written from the reference source and the declared decisions of SURVEY.md (C-1 ... C-13), not from
oracle/ora_pipeline.cpp or host/*.cpp.

The stages are the existing independent restatements: corner_ref.detect (:22), lk_ref.track_features
(feature_tracker.cpp:18-67), stereo_bm_ref.disparity_at (:173-176,193), geom_ref.dedup / triangulate / hmat_from_R_t
(:113-134,178-207), pnp_ref.pnp_ransac (:76-80).  Written here: the tracker's state, the keyframe gate, keyframe assembly,
add_keyframe (refcounts, truncation, ids, the pop), the window gather, the write-back, cv::Rodrigues on the float rvec and
Eigen::Quaternionf(Matrix3f).

THE SOLVE IS A PARAMETER.  tests/ba_ref.py is tolerance-level by design and a window has a gauge, so the bits of ceres::Solve
cannot be restated.  `solve(poses (K, 7), points (N, 3), obs_pose, obs_point, obs_uv (M, 2)) -> (poses, points, iterations)` is
called with the window problem in the declared order (landmark id, then window slot; pose 0 is the constant one,
bundle_adjuster.cpp:130).  The tests pass the oracle's ba_solve: it is pinned to ba_ref in tests/test_ba_ref.py, and the device
solve is bit-identical to it in deterministic mode (ba_max_time_s = 0).

Declared decisions this file follows (the reference as written is undefined or unbounded there):
  C-1  feature_tracker.cpp:58 reads the cleared vector: the OLD id of feature i is meant
  C-2  av_parallax = (sum over the kept) / (number of ALL features); no features at all: 0 instead of 0 / 0
  C-3  refcount = 1 and ++ (:113,116): a landmark's count never returns to 0, avail_ids stays empty, ids are sequential.  Here
       the refcounts and the avail_ids stack are kept as written, and the sequential ids FOLLOW (asserted by the tests)
  C-4  on truncation new_ids holds the real ids only
  C-5  max_features - num_tracked is unsigned (:85): guarded to 0.  From process() the guard cannot fire: after a keyframe the
       tracker holds tracked + new <= max(max_features, tracked) features and only loses some until the next one, so by induction
       num_tracked <= max_features (the counter `c5_guard` stays 0 on every stream; `max_new_zero` is the reachable edge)
  C-7  fewer than 4 corners: the frame is skipped before anything else (:23-25); the tracker's last image stays
  C-9  PnP's return value is ignored; no inliers: a keyframe without tracked features
  C-13 the disparity is read at ((int)x, (int)y)
  rvec / tvec stay float between frames (:54-55); hmat is the evident intent [R^T | -R^T t] (:130-134)
  cv::Rodrigues and the inverse conversion use the declared arithmetic of host/det_trig.h (sincos by polynomial, every operation
  rounded once, evaluated in double, stored as float).  OpenCV groups c1 * (x * y) where det_trig.h declares (c1 * x) * y; the
  declaration is followed.

`variant=` selects one deliberate MISREADING (VARIANTS); the tests show which stream tells each from the reference.
`loss_le` is listed for completeness and is an equivalent mutant: (double) percent_lost is a float and 0.4 is not
(tests/test_pipeline_paths.py::test_loss_le_cannot_differ shows that no count of features makes them equal).
"""
import math

import numpy as np

import corner_ref
import geom_ref
import lk_ref
import pnp_ref
import stereo_bm_ref

F = np.float32
D = np.float64

MIN_DETECTED = 4          # image_processor.cpp:23
PERCENT_LOST = 0.4        # :63, a double literal
PNP_ITERATIONS, PNP_ERROR, PNP_CONFIDENCE = 100, 8.0, 0.99  # :80
NUM_DISPARITIES, BLOCK_SIZE = 16 * 3, 21                    # :174
RODRIGUES_EPS = 2.220446049250313e-16                       # DBL_EPSILON

VARIANTS = ("gate_or", "loss_le", "lost_vs_previous", "all_tracked_into_keyframe", "dedup_all_tracked", "truncate_before_tracked",
            "ids_reused", "pop_late", "hmat_no_transpose", "initial_not_reset", "gather_pose_major")
EQUIVALENT_VARIANTS = ("loss_le",)

COUNTERS = ("skip_before_first", "skip_after_first", "gate_parallax_alone", "gate_loss_alone", "gate_both", "gate_not_taken",
            "percent_lost_nan", "pnp_m0", "pnp_no_model", "inliers_lt_tracked", "dedup_dropped_all", "dedup_dropped_none",
            "new_truncated", "max_new_zero", "c5_guard", "window_popped", "popped_landmark_still_observed", "quat_trace_pos", "quat_x",
            "quat_y", "quat_z", "rodrigues_small")
UNREACHABLE = ("c5_guard", "quat_x", "quat_y")  # C-5 above; x / y need a camera rolled about an image axis (tests/sanitize/det_trig_test.cpp)


# ------------------------------------------------------------------------------------------------ pose conversions
def rodrigues_f(rvec, rec=None):
    """cv::Rodrigues(rvec CV_32F) -> (3, 3) f32 (:84-85): R = c I + (1 - c) r r^T + s [r]x of the unit axis, in double, stored as float."""
    rx, ry, rz = (float(v) for v in np.asarray(rvec, F))
    th = math.sqrt(rx * rx + ry * ry + rz * rz)
    if th < RODRIGUES_EPS:
        if rec is not None:
            rec["rodrigues_small"] += 1
        return np.eye(3, dtype=F)
    s, c = pnp_ref.det_sincos(th)
    c1, it = 1.0 - c, 1.0 / th
    x, y, z = rx * it, ry * it, rz * it
    R = [[c + c1 * x * x, c1 * x * y - s * z, c1 * x * z + s * y],
         [c1 * x * y + s * z, c + c1 * y * y, c1 * y * z - s * x],
         [c1 * x * z - s * y, c1 * y * z + s * x, c + c1 * z * z]]
    return np.array(R, D).astype(F)


def quat_from_R(R, rec=None):
    """Eigen::Quaternionf(Matrix3f) (:92; Eigen/src/Geometry/Quaternion.h, quaternionbase_assign_impl<Other, 3, 3>), every operation in
    f32 -> [w x y z] f32."""
    m = np.asarray(R, F).reshape(3, 3)
    q = np.zeros(4, F)
    t = (m[0, 0] + m[1, 1]) + m[2, 2]
    assert type(t) is F
    if t > F(0):
        t = np.sqrt(t + F(1))
        q[0] = F(0.5) * t
        t = F(0.5) / t
        q[1] = (m[2, 1] - m[1, 2]) * t
        q[2] = (m[0, 2] - m[2, 0]) * t
        q[3] = (m[1, 0] - m[0, 1]) * t
        branch = "quat_trace_pos"
    else:
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        with np.errstate(invalid="ignore", divide="ignore"):
            t = np.sqrt(((m[i, i] - m[j, j]) - m[k, k]) + F(1))
            q[1 + i] = F(0.5) * t
            t = F(0.5) / t
            q[0] = (m[k, j] - m[j, k]) * t
            q[1 + j] = (m[j, i] + m[i, j]) * t
            q[1 + k] = (m[k, i] + m[i, k]) * t
        branch = ("quat_x", "quat_y", "quat_z")[i]
    if rec is not None:
        rec[branch] += 1
    assert q.dtype == F
    return q


# ------------------------------------------------------------------------------------------------ state
class Result:
    """What one frame leaves: the six counts, av_parallax and percent_lost (f32), the last keyframe's float pose as doubles."""
    FIELDS = ("n_detected", "n_tracked", "n_inliers", "n_new", "is_keyframe", "ba_iterations")

    def __init__(self):
        self.n_detected = self.n_tracked = self.n_inliers = self.n_new = self.is_keyframe = self.ba_iterations = 0
        self.av_parallax, self.percent_lost = F(0), F(0)
        self.pose7 = [0.0] * 7


class _Feature:  # bundle_adjuster.hpp:62-72
    def __init__(self):
        self.position, self.refcount = None, 0


class _PoseVariable:  # bundle_adjuster.hpp:49-60
    def __init__(self):
        self.pose = np.zeros(7, D)
        self.observations = []  # (u, v, feature id), in the order the residual blocks were added


class _Keyframe:  # bundle_adjuster.hpp:22-46
    def __init__(self, position, orientation, tracked_2d, tracked_ids, new_2d, new_3d):
        self.position, self.orientation = np.array(position, F), np.array(orientation, F)
        self.tracked_2d, self.tracked_ids = np.array(tracked_2d, F).reshape(-1, 2), list(tracked_ids)
        self.new_2d, self.new_3d, self.new_ids = np.array(new_2d, F).reshape(-1, 2), np.array(new_3d, F).reshape(-1, 3), []


class Pipeline:
    """params: focal, cx, cy, baseline, width, height, max_corners, quality, min_feature_distance, parallax_thresh, window_size,
    max_features (the constructor arguments and `max_features` of the reference).  `problems`, when a list, receives every gathered
    window problem as a dict (poses0, points0, op, oj, uv)."""

    def __init__(self, solve, variant=None, problems=None, **params):
        assert variant is None or variant in VARIANTS, variant
        self.prm, self.solve, self.variant, self.problems = dict(params), solve, variant, problems
        self.rec = dict.fromkeys(COUNTERS, 0)
        # BundleAdjuster
        self.features, self.avail_ids, self.pose_window = [], [], []
        self.last_keyframe, self.new_frame_added = None, False
        self.last_iterations = 0
        # FeatureTracker
        self.last_image, self.initial_features = None, {}
        self.feature_set, self.feature_ids = np.zeros((0, 2), F), []
        # ImageProcessor
        self.rvec, self.tvec = np.zeros(3, F), np.zeros(3, F)

    # -------------------------------------------------------------------------------------------- FeatureTracker
    def _tracker_init(self, image, features, ids):  # feature_tracker.cpp:3-16
        self.feature_ids = list(ids)
        self.feature_set = np.array(features, F).reshape(-1, 2)
        if self.variant != "initial_not_reset":
            self.initial_features = {}                                 # :9
        for i, fid in enumerate(ids):
            self.initial_features.setdefault(fid, self.feature_set[i].copy())  # :11 map::insert keeps the first of an id
        self.last_image = image.copy()

    def _track_features(self, image):  # feature_tracker.cpp:18-67
        n = len(self.feature_ids)
        initial = np.array([self.initial_features[i] for i in self.feature_ids], F).reshape(-1, 2)  # :48-49
        kept_xy, kept_idx, av, _ = lk_ref.track_features(self.last_image, image, self.feature_set, initial)
        old_ids = self.feature_ids
        self.feature_set = kept_xy
        self.feature_ids = [old_ids[i] for i in kept_idx]              # :58, C-1
        size = n if self.variant == "lost_vs_previous" else len(self.initial_features)
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = F(len(self.feature_ids)) / F(size)                 # :64 size_t / float: a float division
        percent_lost = F(1.0 - float(ratio))                           # 1.0 - float: double, stored into the float&
        self.last_image = image.copy()                                 # :66
        return F(av), percent_lost

    # -------------------------------------------------------------------------------------------- BundleAdjuster
    def _remove_oldest_pose(self):  # bundle_adjuster.cpp:41-58
        oldest = self.pose_window[0]
        later = {fid for pv in self.pose_window[1:] for _, _, fid in pv.observations}
        for _, _, fid in oldest.observations:
            self.features[fid].refcount -= 1
            if fid in later:
                self.rec["popped_landmark_still_observed"] += 1
            if self.features[fid].refcount == 0:
                self.avail_ids.append(fid)                             # :50 (never reached as written: C-3)
        self.pose_window.pop(0)
        self.rec["window_popped"] += 1

    def _add_keyframe(self, kf):  # bundle_adjuster.cpp:60-135
        pv = _PoseVariable()
        pv.pose[:4] = kf.orientation.astype(D)                         # :63-66 w x y z
        pv.pose[4:] = kf.position.astype(D)                            # :68-70
        num_tracked = len(kf.tracked_ids)
        for i in range(num_tracked):                                   # :73-83
            fid = kf.tracked_ids[i]
            self.features[fid].refcount += 1
            pv.observations.append((float(kf.tracked_2d[i, 0]), float(kf.tracked_2d[i, 1]), fid))
        max_features = int(self.prm["max_features"])
        if num_tracked > max_features:                                 # :85 unsigned, C-5
            self.rec["c5_guard"] += 1
            max_new = 0
        else:
            max_new = max_features - num_tracked
        if self.variant == "truncate_before_tracked":
            max_new = max_features
        if len(kf.new_2d) > max_new:                                   # :86-90, C-4
            self.rec["new_truncated"] += 1
            self.rec["max_new_zero"] += max_new == 0
            kf.new_2d, kf.new_3d = kf.new_2d[:max_new], kf.new_3d[:max_new]
        for i in range(len(kf.new_2d)):                                # :93-122
            if self.avail_ids:
                fid = self.avail_ids.pop()                             # :101-102 a stack
            else:
                self.features.append(_Feature())
                fid = len(self.features) - 1
            self.features[fid].position = kf.new_3d[i].astype(D)       # :110-112
            self.features[fid].refcount = 1                            # :113
            kf.new_ids.append(fid)
            if self.variant != "ids_reused":
                self.features[fid].refcount += 1                       # :116
            pv.observations.append((float(kf.new_2d[i, 0]), float(kf.new_2d[i, 1]), fid))
        self.pose_window.append(pv)                                    # :125
        if len(self.pose_window) > int(self.prm["window_size"]) + (self.variant == "pop_late"):
            self._remove_oldest_pose()                                 # :126-128
        self.last_keyframe = kf
        self.new_frame_added = True

    def _gather(self):
        """The window problem in the declared order: landmarks by ascending id, each landmark's observations by window slot."""
        flat = [(fid, k, u, v) for k, pv in enumerate(self.pose_window) for u, v, fid in pv.observations]
        if self.variant == "gather_pose_major":
            ids = list(dict.fromkeys(f[0] for f in flat))
        else:
            flat.sort(key=lambda f: (f[0], f[1]))                      # stable: equal (id, slot) keep the order they were added in
            ids = sorted({f[0] for f in flat})
        index = {fid: j for j, fid in enumerate(ids)}
        poses = np.stack([pv.pose for pv in self.pose_window]).astype(D)
        points = np.array([self.features[fid].position for fid in ids], D).reshape(-1, 3)
        op = np.array([f[1] for f in flat], np.int32)
        oj = np.array([index[f[0]] for f in flat], np.int32)
        uv = np.array([[f[2], f[3]] for f in flat], D).reshape(-1, 2)
        return ids, poses, points, op, oj, uv

    def _bundle_adjust(self):  # bundle_adjuster.cpp:137-157
        self.last_iterations = 0
        if not self.new_frame_added:
            return
        ids, poses, points, op, oj, uv = self._gather()
        if self.problems is not None:
            self.problems.append(dict(poses0=poses.copy(), points0=points.copy(), op=op.copy(), oj=oj.copy(), uv=uv.copy()))
        poses, points, iterations = self.solve(poses, points, op, oj, uv)
        self.last_iterations = int(iterations)
        for k, pv in enumerate(self.pose_window):                      # ceres solves in place
            pv.pose = np.array(poses[k], D)
        for j, fid in enumerate(ids):
            self.features[fid].position = np.array(points[j], D)
        back = self.pose_window[-1].pose                               # :146-153 doubles stored into the Keyframe's floats
        self.last_keyframe.orientation = back[:4].astype(F)
        self.last_keyframe.position = back[4:].astype(F)
        self.new_frame_added = False

    # -------------------------------------------------------------------------------------------- ImageProcessor
    def _triangulate_stereo(self, features_2d, left, right, camera_pose):  # image_processor.cpp:165-208
        p = self.prm
        features_2d = np.array(features_2d, F).reshape(-1, 2)
        if len(features_2d) == 0:
            return np.zeros((0, 2), F), np.zeros((0, 3), F)
        disp = stereo_bm_ref.disparity_at(left, right, features_2d, NUM_DISPARITIES, BLOCK_SIZE)
        kept_xy, xyz, _ = geom_ref.triangulate(features_2d, disp, camera_pose, p["focal"], p["cx"], p["cy"], p["baseline"])
        return kept_xy, xyz

    def _process(self, left, right, res):  # image_processor.cpp:18-163
        p, rec = self.prm, self.rec
        detected = corner_ref.detect(left, int(p["max_corners"]), p["quality"], p["min_feature_distance"])  # :22
        res.n_detected = len(detected)
        if len(detected) < MIN_DETECTED:                               # :23-25
            rec["skip_after_first" if self.last_keyframe is not None else "skip_before_first"] += 1
            return
        if self.last_keyframe is None:                                 # :30-58
            new_2d, new_3d = self._triangulate_stereo(detected, left, right, np.eye(4, dtype=F))
            kf = _Keyframe(np.zeros(3, F), np.array([1, 0, 0, 0], F), [], [], new_2d, new_3d)
            self._add_keyframe(kf)
            self._tracker_init(left, kf.new_2d, kf.new_ids)
            self.tvec, self.rvec = np.zeros(3, F), np.zeros(3, F)
            res.is_keyframe, res.n_new = 1, len(kf.new_ids)
            return
        av_parallax, percent_lost = self._track_features(left)         # :62
        res.n_tracked, res.av_parallax, res.percent_lost = len(self.feature_ids), av_parallax, percent_lost
        rec["percent_lost_nan"] += bool(np.isnan(percent_lost))
        small = bool(av_parallax <= F(p["parallax_thresh"]))           # :63 float <= float
        few_lost = bool(float(percent_lost) <= PERCENT_LOST) if self.variant == "loss_le" else bool(float(percent_lost) < PERCENT_LOST)
        if (small or few_lost) if self.variant == "gate_or" else (small and few_lost):
            rec["gate_not_taken"] += 1
            return                                                     # :64
        rec["gate_both" if not small and not few_lost else "gate_parallax_alone" if not small else "gate_loss_alone"] += 1
        tracked_features, tracked_ids = self.feature_set, self.feature_ids             # :71
        world = np.array([self.features[i].position for i in tracked_ids], D).reshape(-1, 3).astype(F)  # :72, bundle_adjuster.cpp:161
        m = len(tracked_ids)
        rec["pnp_m0"] += m == 0
        rv, tv, inliers, prec = pnp_ref.pnp_ransac(world, tracked_features, p["focal"], p["cx"], p["cy"], self.rvec.astype(D),
                                                   self.tvec.astype(D), PNP_ITERATIONS, PNP_ERROR, PNP_CONFIDENCE)  # :76-80
        self.rvec, self.tvec = np.asarray(rv, D).astype(F), np.asarray(tv, D).astype(F)
        rec["pnp_no_model"] += prec["best"] < 0
        num_inliers = len(inliers)                                     # :82
        rec["inliers_lt_tracked"] += 0 < num_inliers < m
        res.n_inliers = num_inliers
        rmat = rodrigues_f(self.rvec, rec)                             # :84-85
        orientation = quat_from_R(rmat, rec)                           # :92
        if self.variant == "all_tracked_into_keyframe":
            inliers = np.arange(m)
        kf = _Keyframe(self.tvec, orientation, tracked_features[inliers], [tracked_ids[i] for i in inliers], [], [])  # :95-108
        against = tracked_features if self.variant == "dedup_all_tracked" else kf.tracked_2d
        new_features = geom_ref.dedup(detected, against, p["min_feature_distance"])     # :113-128
        if len(against):
            rec["dedup_dropped_all"] += len(new_features) == 0
            rec["dedup_dropped_none"] += len(new_features) == len(detected)
        if self.variant == "hmat_no_transpose":
            hmat = geom_ref.hmat_from_R_t(rmat.T.copy(), self.tvec)    # [R | -R t]
        else:
            hmat = geom_ref.hmat_from_R_t(rmat, self.tvec)             # :130-134
        kf.new_2d, kf.new_3d = self._triangulate_stereo(new_features, left, right, hmat)  # :137-142
        self._add_keyframe(kf)                                         # :144
        features = np.concatenate([kf.tracked_2d, kf.new_2d])          # :148-161
        self._tracker_init(left, features, kf.tracked_ids + kf.new_ids)  # :162
        res.is_keyframe, res.n_new = 1, len(kf.new_ids)

    # -------------------------------------------------------------------------------------------- the driver
    def process(self, left, right):
        """One frame: process(), then bundle_adjust() if a keyframe exists (vo_node.cpp:141-148).  Returns a Result."""
        left, right = np.ascontiguousarray(left, np.uint8), np.ascontiguousarray(right, np.uint8)
        res = Result()
        self._process(left, right, res)
        if self.last_keyframe is not None:                             # vo_node.cpp:146-148
            self._bundle_adjust()
            res.ba_iterations = self.last_iterations
            res.pose7 = [float(v) for v in self.last_keyframe.orientation] + [float(v) for v in self.last_keyframe.position]
        return res

    def tracked(self):
        """The tracker's list (feature_tracker.cpp:69-72): ids (n,) int64, positions (n, 2) f32."""
        return np.array(self.feature_ids, np.int64), np.array(self.feature_set, F).reshape(-1, 2)
