"""ctypes binding of include/svo.h.  Mirrors the C-ABI one to one; numpy arrays in, numpy arrays out."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


class SvoError(RuntimeError):
    pass


def lib_path():
    return os.path.join(_HERE, "libsvo_hip.so")


class Limits(C.Structure):
    _fields_ = [("max_width", C.c_int), ("max_height", C.c_int), ("max_batch", C.c_int),
                ("max_corners", C.c_int), ("max_candidates", C.c_int), ("max_features", C.c_int)]


class CameraInfo(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("focal", "cx", "cy", "k1", "k2", "p1", "p2", "baseline")]


class RectifyEye(C.Structure):
    """svo_rectify_eye: one RAW camera (matrix, Brown-Conrady k1 k2 p1 p2, rotation raw -> rectified, row-major)."""
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("k1", C.c_double), ("k2", C.c_double), ("p1", C.c_double), ("p2", C.c_double), ("R", C.c_double * 9)]


def rectify_eye(fx, fy, cx, cy, k1=0.0, k2=0.0, p1=0.0, p2=0.0, R=None):
    R = np.eye(3) if R is None else np.asarray(R, np.float64).reshape(3, 3)
    return RectifyEye(fx, fy, cx, cy, k1, k2, p1, p2, (C.c_double * 9)(*R.reshape(-1)))


def rectify_eye_from_camera_info(cam):
    """svo_rectify_eye_from_camera_info: the monocular case (fx = fy = focal, same centre, R = I)."""
    e = RectifyEye()
    if lib().svo_rectify_eye_from_camera_info(C.byref(cam), C.byref(e)) != 0:
        raise SvoError("svo_rectify_eye_from_camera_info failed")
    return e


def rectify_build_map(eye, cam, width, height):
    """svo_rectify_build_map (host only): (height, width, 2) int16 records (dx, dy) in 1/32 px, (-32768, -32768) = no source."""
    L = lib()
    out = np.empty((height, width, 2), np.int16)
    rc = L.svo_rectify_build_map(C.byref(eye), C.byref(cam), width, height, _p(out))
    if rc:
        raise SvoError(f"svo_rectify_build_map rc={rc}: {L.svo_last_error(None).decode()}")
    return out


class BAOptions(C.Structure):
    _fields_ = [("max_iterations", C.c_int), ("max_time_s", C.c_double),
                ("function_tolerance", C.c_double), ("gradient_tolerance", C.c_double),
                ("parameter_tolerance", C.c_double), ("initial_radius", C.c_double),
                ("max_features", C.c_int), ("accumulation", C.c_int)]


BA_ACC = {"auto": 0, "deterministic": 1, "atomics": 2, "mfma": 3}


class BASummary(C.Structure):
    _fields_ = [("iterations", C.c_int), ("successful_steps", C.c_int), ("termination", C.c_int),
                ("initial_cost", C.c_double), ("final_cost", C.c_double), ("solve_ms", C.c_double)]


class PipelineParams(C.Structure):
    _fields_ = [("cam", CameraInfo), ("width", C.c_int), ("height", C.c_int), ("max_corners", C.c_int),
                ("quality", C.c_double), ("min_feature_distance", C.c_float),
                ("parallax_thresh", C.c_float), ("window_size", C.c_int), ("max_features", C.c_int),
                ("ba_max_iterations", C.c_int), ("ba_max_time_s", C.c_double)]


class FrameResult(C.Structure):
    _fields_ = [("n_detected", C.c_int), ("n_tracked", C.c_int), ("n_inliers", C.c_int),
                ("n_new", C.c_int), ("is_keyframe", C.c_int), ("av_parallax", C.c_float),
                ("percent_lost", C.c_float), ("pose7", C.c_double * 7), ("ba_iterations", C.c_int)]


class CloudParams(C.Structure):
    """svo_cloud_params: which pixels of a disparity map become points, and how many are stored per image."""
    _fields_ = [("step", C.c_int), ("min_disparity", C.c_float), ("max_points", C.c_int)]


class CloudPoint(C.Structure):
    """svo_cloud_point: 16 bytes; tag = (y * width + x) | (left[y][x] << 24)."""
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float), ("tag", C.c_uint32)]


class SpeckleParams(C.Structure):
    """svo_speckle_params: components of at most max_size pixels go; neighbours join iff |a - b| <= max_diff16 (1/16 px)."""
    _fields_ = [("max_size", C.c_int), ("max_diff16", C.c_int)]


class LrCheckParams(C.Structure):
    """svo_lr_check_params: a pixel goes iff both of its right-view look-ups differ from it by more than max_diff16 (1/16 px)."""
    _fields_ = [("max_diff16", C.c_int)]


class SgmParams(C.Structure):
    """svo_sgm_params: the penalties of semi-global matching, 0 <= p1 <= p2 <= SGM_MAX_P2."""
    _fields_ = [("p1", C.c_int), ("p2", C.c_int)]


LR_CHECK_MAX_WIDTH = 10240  # SVO_LR_CHECK_MAX_WIDTH
SGM_MAX_P2 = 32767  # SVO_SGM_MAX_P2
SGM_KEYFRAME_SUB_BATCH = 2  # SVO_SGM_KEYFRAME_SUB_BATCH


def sgm_default_params(block=21):
    """svo_sgm_default_params: p1 = 2 block^2, p2 = 8 block^2 (chosen on a synthetic scene, not tuned on real imagery)."""
    prm = SgmParams()
    if lib().svo_sgm_default_params(C.byref(prm), int(block)) != 0:
        raise SvoError(f"svo_sgm_default_params: block_size {block} is not odd 5..21")
    return prm


def sgm_workspace_bytes(width, height, ndisp=48, block=21, batch=1):
    """svo_sgm_workspace_bytes: device bytes semi-global matching needs for `batch` pairs (no GPU involved); 0: a refused shape."""
    return int(lib().svo_sgm_workspace_bytes(width, height, ndisp, block, batch))


def _sgm_params(p1, p2, block=21):
    prm = sgm_default_params(block)
    if p1 is not None:
        prm.p1 = int(p1)
    if p2 is not None:
        prm.p2 = int(p2)
    return prm


class VoxelMapParams(C.Structure):
    """svo_voxel_map_params: voxel edge (finite, > 0), table of 2^capacity_log2 slots (8..28), max_depth <= 0 = no depth bound."""
    _fields_ = [("voxel_size", C.c_float), ("capacity_log2", C.c_int), ("max_depth", C.c_float)]


class VoxelMapStats(C.Structure):
    """svo_voxel_map_stats_t: slots claimed, and points inserted / rejected / dropped."""
    _fields_ = [("n_voxels", C.c_uint64), ("n_inserted", C.c_uint64), ("n_rejected", C.c_uint64), ("n_dropped", C.c_uint64)]


VOXEL_MAX_PROBES = 64  # SVO_VOXEL_MAX_PROBES


def _params(default, given, **overrides):
    """A copy of `given` (or default() when it is None), then the overrides that are not None, each as its field's own type."""
    prm = default()
    for name, _ in prm._fields_:
        if given is not None:
            setattr(prm, name, getattr(given, name))
        if overrides.get(name) is not None:
            setattr(prm, name, type(getattr(prm, name))(overrides[name]))
    return prm


def voxel_map_default_params():
    """svo_voxel_map_default_params: voxel_size 0.1, capacity_log2 22, max_depth 0."""
    p = VoxelMapParams()
    if lib().svo_voxel_map_default_params(C.byref(p)) != 0:
        raise SvoError("svo_voxel_map_default_params failed")
    return p


def voxel_map_bytes(params):
    """svo_voxel_map_bytes: bytes of the table, 40 per slot (no GPU involved); raises for parameters the map refuses."""
    n = C.c_size_t(0)
    if lib().svo_voxel_map_bytes(C.byref(params), C.byref(n)) != 0:
        raise SvoError("svo_voxel_map_bytes: voxel_size must be finite and > 0, capacity_log2 in 8..28")
    return int(n.value)


def pose7_to_cam_to_world(pose7):
    """svo_pose7_to_cam_to_world: [qw qx qy qz tx ty tz] (X_cam = R(q) X_world + t) -> the (3, 4) f64 camera->world matrix [R^T | -R^T t]."""
    q = _f64(pose7).reshape(7)
    m = np.empty((3, 4), np.float64)
    if lib().svo_pose7_to_cam_to_world(_p(q), _p(m)) != 0:
        raise SvoError("svo_pose7_to_cam_to_world failed")
    return m


class VoxelLedgerParams(C.Structure):
    """svo_voxel_ledger_params: clouds held at once (>= 1), records per cloud (>= 1)."""
    _fields_ = [("max_keyframes", C.c_int), ("max_points", C.c_int)]


def voxel_ledger_bytes(max_keyframes, max_points):
    """svo_voxel_ledger_bytes: 16 * max_keyframes * max_points (no GPU involved); raises for parameters the ledger refuses."""
    n = C.c_size_t(0)
    if lib().svo_voxel_ledger_bytes(C.byref(VoxelLedgerParams(int(max_keyframes), int(max_points))), C.byref(n)) != 0:
        raise SvoError("svo_voxel_ledger_bytes: max_keyframes and max_points must be at least 1")
    return int(n.value)


REMOVE_COUNTS = ("n_removed", "n_rejected", "n_missing", "n_short")


class VoxelCarveParams(C.Structure):
    """svo_voxel_carve_params: window half width (0..3), margin in sixteenths of disparity (0..32767), keep_count (0 = off)."""
    _fields_ = [("radius", C.c_int), ("margin16", C.c_int), ("keep_count", C.c_int)]


def voxel_carve_default_params():
    """svo_voxel_carve_default_params: radius 1, margin16 8, keep_count 0 (not tuned on real imagery)."""
    p = VoxelCarveParams()
    if lib().svo_voxel_carve_default_params(C.byref(p)) != 0:
        raise SvoError("svo_voxel_carve_default_params failed")
    return p


def _carve_params(params, radius, margin16, keep_count):
    return _params(voxel_carve_default_params, params, radius=radius, margin16=margin16, keep_count=keep_count)


def pose7_to_world_to_cam(pose7):
    """svo_pose7_to_world_to_cam: [qw qx qy qz tx ty tz] (X_cam = R(q) X_world + t) -> the (3, 4) f64 world->camera matrix [R | t]."""
    q = _f64(pose7).reshape(7)
    m = np.empty((3, 4), np.float64)
    if lib().svo_pose7_to_world_to_cam(_p(q), _p(m)) != 0:
        raise SvoError("svo_pose7_to_world_to_cam failed")
    return m


class VoxelRenderParams(C.Structure):
    """svo_voxel_render_params: min_count (>= 1), bound on the footprint's half width in pixels (0..16)."""
    _fields_ = [("min_count", C.c_int), ("max_radius", C.c_int)]


def voxel_render_default_params():
    """svo_voxel_render_default_params: min_count 1, max_radius 8 (not tuned on real imagery)."""
    p = VoxelRenderParams()
    if lib().svo_voxel_render_default_params(C.byref(p)) != 0:
        raise SvoError("svo_voxel_render_default_params failed")
    return p


def voxel_render_workspace_bytes(width, height):
    """svo_voxel_render_workspace_bytes: 4 * width * height (no GPU involved); 0 for width or height < 1."""
    return int(lib().svo_voxel_render_workspace_bytes(int(width), int(height)))


def _render_params(params, min_count, max_radius):
    return _params(voxel_render_default_params, params, min_count=min_count, max_radius=max_radius)


class VoxelAlignParams(C.Structure):
    """svo_voxel_align_params: min_count (>= 1), reach (0 or 1), max_dist (finite, in (0, 8]), max_iters (>= 1), min_matches (>= 6),
    eps_t and eps_r (finite, >= 0)."""
    _fields_ = [("min_count", C.c_int), ("reach", C.c_int), ("max_dist", C.c_float), ("max_iters", C.c_int), ("min_matches", C.c_int),
                ("eps_t", C.c_float), ("eps_r", C.c_float)]


class VoxelAlignResult(C.Structure):
    """svo_voxel_align_result."""
    _fields_ = [("status", C.c_int), ("iterations", C.c_int), ("first_matched", C.c_int64), ("last_matched", C.c_int64),
                ("first_cost", C.c_int64), ("last_cost", C.c_int64), ("xi", C.c_double * 6)]


VOXEL_ALIGN_WORDS = 32  # SVO_VOXEL_ALIGN_WORDS: int64 words of `sums`
VOXEL_ALIGN_MAX_POINTS = 1 << 20
VOXEL_ALIGN_STATUS = ("CONVERGED", "MAX_ITERS", "TOO_FEW", "DEGENERATE")  # SVO_VOXEL_ALIGN_*, by value
ALIGN_COUNTS = ("n_matched", "n_rejected", "n_unmatched", "n_far")  # words 17..20 of the sums


def _align_result(res):
    """A VoxelAlignResult as the dict VoxelMap.align and .align_plane return."""
    return {"status": VOXEL_ALIGN_STATUS[res.status], "iterations": res.iterations, "first_matched": int(res.first_matched),
            "last_matched": int(res.last_matched), "first_cost": int(res.first_cost), "last_cost": int(res.last_cost),
            "xi": np.array(list(res.xi), np.float64)}


def voxel_align_default_params(voxel_size):
    """svo_voxel_align_default_params: min_count 1, reach 1, max_dist 2 * voxel_size (at most 8), max_iters 10, min_matches 64,
    eps_t voxel_size / 100, eps_r 1e-5 (not tuned on real imagery)."""
    p = VoxelAlignParams()
    if lib().svo_voxel_align_default_params(C.c_float(voxel_size), C.byref(p)) != 0:
        raise SvoError("svo_voxel_align_default_params: voxel_size must be finite and > 0")
    return p


class VoxelNormalsParams(C.Structure):
    """svo_voxel_normals_params: min_count (>= 1), min_neighbours (3..27), max_curvature (finite, in (0, 1])."""
    _fields_ = [("min_count", C.c_int), ("min_neighbours", C.c_int), ("max_curvature", C.c_float)]


VoxelNormal = np.dtype([("nx", np.float32), ("ny", np.float32), ("nz", np.float32), ("curvature", np.float32)])  # svo_voxel_normal
NORMALS_COUNTS = ("n_centres", "n_valid", "n_few", "n_collinear", "n_curved")  # words 0..4 of the 8 counts; the rest stay zero
VOXEL_NORMALS_COUNTS = 8  # SVO_VOXEL_NORMALS_COUNTS: uint64 words of `counts`
VOXEL_ALIGN_PLANE_WORDS = 40  # SVO_VOXEL_ALIGN_PLANE_WORDS: int64 words of the plane form's `sums`
ALIGN_PLANE_COUNTS = ("n_matched", "n_rejected", "n_unmatched", "n_far", "n_no_normal")  # words 29..33 of the plane form's sums


def voxel_normals_default_params():
    """svo_voxel_normals_default_params: min_count 1, min_neighbours 5, max_curvature 1.0 (not tuned on real imagery)."""
    p = VoxelNormalsParams()
    if lib().svo_voxel_normals_default_params(C.byref(p)) != 0:
        raise SvoError("svo_voxel_normals_default_params failed")
    return p


def voxel_map_normals_bytes(params):
    """svo_voxel_map_normals_bytes: bytes of a map's side array of normals, 16 per slot (no GPU involved); params: a VoxelMapParams."""
    n = C.c_size_t(0)
    if lib().svo_voxel_map_normals_bytes(C.byref(params), C.byref(n)) != 0:
        raise SvoError("svo_voxel_map_normals_bytes: voxel_size must be finite and > 0, capacity_log2 in 8..28")
    return int(n.value)


class VoxelLocateParams(C.Structure):
    """svo_voxel_locate_params: min_count (>= 1), up_axis (0..2), n_turn (0..31), turn_step (finite, in (0, 0.25]), box[3] (each
    0..16), dims[3] (each 1..2048, dims[0] a multiple of 64, product <= 2^30), n_refine (1..63), min_hits (>= 1)."""
    _fields_ = [("min_count", C.c_int), ("up_axis", C.c_int), ("n_turn", C.c_int), ("turn_step", C.c_float), ("box", C.c_int * 3),
                ("dims", C.c_int * 3), ("n_refine", C.c_int), ("min_hits", C.c_int)]


class VoxelLocateResult(C.Structure):
    """svo_voxel_locate_result."""
    _fields_ = [("status", C.c_int), ("k", C.c_int), ("shift", C.c_int * 3), ("hits", C.c_uint32), ("rank", C.c_int), ("n_refined", C.c_int),
                ("coarse_pose7", C.c_double * 7), ("align", VoxelAlignResult)]


VoxelLocateBest = np.dtype([("hits_max", np.uint32), ("s0", np.int32), ("s1", np.int32), ("s2", np.int32), ("n_used", np.uint32),
                            ("n_inside", np.uint32), ("index", np.uint32), ("zero", np.uint32)])  # svo_voxel_locate_best, 32 bytes
VOXEL_LOCATE_STATUS = ("FOUND", "UNREFINED", "NO_CANDIDATE")  # SVO_VOXEL_LOCATE_*, by value
VOXEL_LOCATE_CHUNK = 1024  # records per workgroup of the score launch (host/voxel_locate.h): the tests straddle it
OCCUPANCY_COUNTS = ("n_inside", "n_outside")


def _int3(v):
    a = np.ascontiguousarray(v, dtype=np.int32)
    if a.shape != (3,):
        raise ValueError("three integers wanted")
    return a


def voxel_locate_default_params(voxel_size):
    """svo_voxel_locate_default_params: min_count 1, up_axis 1, n_turn 4, turn_step 0.04, box (8, 4, 8), dims (512, 128, 512),
    n_refine 3, min_hits 64 (not tuned on real imagery)."""
    p = VoxelLocateParams()
    if lib().svo_voxel_locate_default_params(C.c_float(voxel_size), C.byref(p)) != 0:
        raise SvoError("svo_voxel_locate_default_params: voxel_size must be finite and > 0")
    return p


def voxel_locate_workspace_bytes(params):
    """svo_voxel_locate_workspace_bytes: bytes of the workspace VoxelMap.locate wants (no GPU involved); params: a VoxelLocateParams."""
    n = C.c_size_t(0)
    if lib().svo_voxel_locate_workspace_bytes(C.byref(params), C.byref(n)) != 0:
        raise SvoError("svo_voxel_locate_workspace_bytes: parameters svo_voxel_map_locate refuses")
    return int(n.value)


def voxel_occupancy_bytes(dims):
    """svo_voxel_occupancy_bytes: bytes of an occupancy volume of dims = (d0, d1, d2) voxels, one bit each (no GPU involved)."""
    n = C.c_size_t(0)
    if lib().svo_voxel_occupancy_bytes(_p(_int3(dims)), C.byref(n)) != 0:
        raise SvoError("svo_voxel_occupancy_bytes: each dimension in 1..2048, dims[0] a multiple of 64, the product at most 2^30")
    return int(n.value)


class VoxelRaycastParams(C.Structure):
    """svo_voxel_raycast_params: max_range (finite, >= 0, metres along the ray), min_step (0..255: cells visited before this step are
    not tested)."""
    _fields_ = [("max_range", C.c_float), ("min_step", C.c_int)]


VoxelRay = np.dtype([("ox", np.float32), ("oy", np.float32), ("oz", np.float32), ("max_range", np.float32), ("dx", np.float32),
                     ("dy", np.float32), ("dz", np.float32), ("tag", np.uint32)])  # svo_voxel_ray, 32 bytes
VoxelRayHit = np.dtype([("cell", np.uint32), ("steps", np.uint32), ("dist", np.float32), ("status", np.uint32)])  # svo_voxel_ray_hit, 16 bytes
VOXEL_RAY_STATUS = ("HIT", "LEFT", "RANGE", "OUTSIDE", "REJECTED")  # SVO_VOXEL_RAY_*, by value: status & 255; status >> 8 is the axis
RAYS_COUNTS = ("n_hit", "n_left", "n_range", "n_outside", "n_rejected", "n_steps")
RAYCAST_COUNTS = RAYS_COUNTS + ("n_pixels",)
VOXEL_RAYS_MAX = 1 << 20


def voxel_raycast_default_params():
    """svo_voxel_raycast_default_params: max_range 30.0, min_step 1 (not tuned on real imagery)."""
    p = VoxelRaycastParams()
    if lib().svo_voxel_raycast_default_params(C.byref(p)) != 0:
        raise SvoError("svo_voxel_raycast_default_params failed")
    return p


def voxel_occupancy_coarse_bytes(dims):
    """svo_voxel_occupancy_coarse_bytes: bytes of the coarse volume of an occupancy volume of dims voxels, one bit per 8 x 8 x 8 block
    (no GPU involved)."""
    n = C.c_size_t(0)
    if lib().svo_voxel_occupancy_coarse_bytes(_p(_int3(dims)), C.byref(n)) != 0:
        raise SvoError("svo_voxel_occupancy_coarse_bytes: each dimension in 1..2048, dims[0] a multiple of 64, the product at most 2^30")
    return int(n.value)


class VoxelDistanceParams(C.Structure):
    """svo_voxel_distance_params: max_dist (1..254 voxels: farther sources are not looked for), inflate_radius (finite, >= 0, map
    units: the radius of the inflated volume)."""
    _fields_ = [("max_dist", C.c_int), ("inflate_radius", C.c_float)]


class VoxelDistanceOut(C.Structure):
    """svo_voxel_distance_out: dist2 (uint16 per cell, required), nearest (uint32 per cell), clearance (float32 per cell), inflated
    (uint64 words of the occupancy's layout); the last three may be None."""
    _fields_ = [("dist2", C.c_void_p), ("nearest", C.c_void_p), ("clearance", C.c_void_p), ("inflated", C.c_void_p)]


VoxelSphere = np.dtype([("x", np.float32), ("y", np.float32), ("z", np.float32), ("radius", np.float32)])  # svo_voxel_sphere, 16 bytes
VoxelSphereHit = np.dtype([("cell", np.uint32), ("dist2", np.uint32), ("clearance", np.float32), ("code", np.uint32)])  # svo_voxel_sphere_hit, 16 bytes
VOXEL_SPHERE_CODE = ("FREE", "COLLIDES", "OUTSIDE", "REJECTED")  # SVO_VOXEL_SPHERE_*, by value
DISTANCE_COUNTS = ("n_sources", "n_reached", "n_unreached", "n_inflated")
DISTANCE_QUERY_COUNTS = ("n", "n_free", "n_collides", "n_outside", "n_rejected", "n_beyond")
VOXEL_DISTANCE_NONE16 = 0xFFFF
VOXEL_DISTANCE_QUERY_MAX = 1 << 20


def voxel_distance_default_params(voxel_size):
    """svo_voxel_distance_default_params: max_dist 32 voxels, inflate_radius 0 (not tuned on real data)."""
    p = VoxelDistanceParams()
    if lib().svo_voxel_distance_default_params(C.c_float(voxel_size), C.byref(p)) != 0:
        raise SvoError("svo_voxel_distance_default_params: voxel_size must be finite and > 0")
    return p


def voxel_distance_workspace_bytes(dims, want_nearest=False):
    """svo_voxel_distance_workspace_bytes: bytes of the workspace VoxelMap.distance wants for a volume of dims voxels, 3 per cell, or 6
    when nearest is asked for (no GPU involved)."""
    n = C.c_size_t(0)
    if lib().svo_voxel_distance_workspace_bytes(_p(_int3(dims)), int(bool(want_nearest)), C.byref(n)) != 0:
        raise SvoError("svo_voxel_distance_workspace_bytes: each dimension in 1..2048, dims[0] a multiple of 64, the product at most 2^30")
    return int(n.value)


def voxel_distance_bytes(dims):
    """svo_voxel_distance_bytes: bytes of the dist2 output for a volume of dims voxels, 2 per cell (no GPU involved)."""
    n = C.c_size_t(0)
    if lib().svo_voxel_distance_bytes(_p(_int3(dims)), C.byref(n)) != 0:
        raise SvoError("svo_voxel_distance_bytes: each dimension in 1..2048, dims[0] a multiple of 64, the product at most 2^30")
    return int(n.value)


class VoxelRouteParams(C.Structure):
    """svo_voxel_route_params: the penalty's squared radius in voxels (0..254^2) and its weight (near_weight * near_r2 <= 2^20), the
    cap on a cell's cost (1..0x7F000000), the relaxation rounds one call enqueues (1..4096), the cells written per path (1..2^20,
    read only with starts) and resume (0 or 1)."""
    _fields_ = [("near_r2", C.c_uint32), ("near_weight", C.c_uint32), ("max_cost", C.c_uint32), ("max_rounds", C.c_int), ("max_path", C.c_int),
                ("resume", C.c_int)]


class VoxelRouteOut(C.Structure):
    """svo_voxel_route_out: cost and next d0*d1*d2 elements, path n_starts x max_path, path_len and path_status n_starts; every pointer
    but cost may be None, the three path pointers only together."""
    _fields_ = [("cost", C.c_void_p), ("next", C.c_void_p), ("path", C.c_void_p), ("path_len", C.c_void_p), ("path_status", C.c_void_p)]


VOXEL_ROUTE_NONE = 0xFFFFFFFF  # SVO_VOXEL_ROUTE_NONE
VOXEL_ROUTE_MAX_COST = 0x7F000000  # SVO_VOXEL_ROUTE_MAX_COST
VOXEL_ROUTE_COUNTS = ("n_goals_used", "n_reached", "n_unreached", "n_closed", "converged", "rounds_run")
VOXEL_ROUTE_OK, VOXEL_ROUTE_TRUNCATED, VOXEL_ROUTE_UNREACHED, VOXEL_ROUTE_OUT_OF_VOLUME, VOXEL_ROUTE_NOT_CONVERGED = range(5)
VOXEL_ROUTE_SELF = 13  # next at a used goal


def voxel_route_default_params(voxel_size):
    """svo_voxel_route_default_params: no penalty, max_cost 0x7F000000, 32 rounds, paths of up to 4096 cells, resume 0 (not tuned on
    real data)."""
    p = VoxelRouteParams()
    if lib().svo_voxel_route_default_params(C.c_float(voxel_size), C.byref(p)) != 0:
        raise SvoError("svo_voxel_route_default_params: voxel_size must be finite and > 0")
    return p


def voxel_route_workspace_bytes(dims):
    """svo_voxel_route_workspace_bytes: bytes of the workspace VoxelMap.route wants for a volume of dims voxels: a header, two words
    per tile and a byte per cell (no GPU involved)."""
    n = C.c_size_t(0)
    if lib().svo_voxel_route_workspace_bytes(_p(_int3(dims)), C.byref(n)) != 0:
        raise SvoError("svo_voxel_route_workspace_bytes: each dimension in 1..2048, dims[0] a multiple of 64, the product at most 2^30")
    return int(n.value)


def voxel_occupancy_cell_of(voxel_size, origin, dims, xyz):
    """svo_voxel_occupancy_cell_of: the cell number j0 + d0 * (j1 + d1 * j2) of the world position xyz (three float32, map units) in the
    volume of origin and dims, by the distance query's rule; what route() takes as goals and starts.  Raises SvoError for a position
    outside the volume or the key range and for refused arguments (no GPU involved)."""
    x = np.ascontiguousarray(xyz, np.float32).ravel()
    if x.size != 3:
        raise ValueError("voxel_occupancy_cell_of: xyz must hold three values")
    cell = C.c_uint32(0)
    if lib().svo_voxel_occupancy_cell_of(C.c_float(voxel_size), _p(_int3(origin)), _p(_int3(dims)), _p(x), C.byref(cell)) != 0:
        raise SvoError("svo_voxel_occupancy_cell_of: the position is outside the volume or the key range, or an argument is refused")
    return int(cell.value)


class VoxelGridParams(C.Structure):
    """svo_voxel_grid_params: up_axis (0..2), up_sign (+1 / -1), the corner of cell (0, 0) in map units, voxels per cell edge
    (1..1024), na x nb cells (each 1..8192, na*nb <= 2^24), the height band, the span beyond which a cell is an obstacle, min_count."""
    _fields_ = [("up_axis", C.c_int), ("up_sign", C.c_int), ("origin_a", C.c_double), ("origin_b", C.c_double), ("cell_voxels", C.c_int),
                ("na", C.c_int), ("nb", C.c_int), ("up_lo", C.c_double), ("up_hi", C.c_double), ("obstacle_step", C.c_double),
                ("min_count", C.c_int)]


class VoxelGridOut(C.Structure):
    """svo_voxel_grid_out: na*nb elements each; every pointer but cls may be None."""
    _fields_ = [("cls", C.c_void_p), ("top", C.c_void_p), ("bottom", C.c_void_p), ("intensity", C.c_void_p), ("n_voxels", C.c_void_p),
                ("n_points", C.c_void_p)]


VOXEL_GRID_UNKNOWN, VOXEL_GRID_LEVEL, VOXEL_GRID_OBSTACLE = 0, 1, 2
GRID_PRECHECK_DEFAULT = False  # svo_voxel_grid_set_mode's state of a new map
GRID_COUNTS = ("n_qualifying", "n_in_band", "n_binned", "n_cells", "n_obstacle")


def voxel_grid_default_params(voxel_size):
    """svo_voxel_grid_default_params: the camera convention (y down), 0.5-unit cells, 256 x 256 of them starting at a = 0 and centred
    on b = 0, the band -3 .. 2.5, obstacle_step 0.3, min_count 1 (not tuned on real imagery)."""
    p = VoxelGridParams()
    if lib().svo_voxel_grid_default_params(C.c_float(voxel_size), C.byref(p)) != 0:
        raise SvoError("svo_voxel_grid_default_params: voxel_size must be finite and > 0")
    return p


def voxel_grid_workspace_bytes(na, nb):
    """svo_voxel_grid_workspace_bytes: 32 * na * nb (no GPU involved); 0 for na or nb < 1."""
    return int(lib().svo_voxel_grid_workspace_bytes(int(na), int(nb)))


def voxel_grid_cell_of(params, voxel_size, a, b):
    """svo_voxel_grid_cell_of: (inside, ia, ib) of the position (a, b) in map units along the grid's axes, by the grid's own rule."""
    ia, ib = C.c_int(0), C.c_int(0)
    rc = lib().svo_voxel_grid_cell_of(C.byref(params), C.c_float(voxel_size), C.c_double(a), C.c_double(b), C.byref(ia), C.byref(ib))
    if rc < 0:
        raise SvoError("svo_voxel_grid_cell_of: refused parameters, voxel_size or a NaN position")
    return bool(rc), ia.value, ib.value


def _grid_params(voxel_size, params, overrides):
    return _params(lambda: voxel_grid_default_params(voxel_size), params, **overrides)


class GridClearanceParams(C.Structure):
    """svo_grid_clearance_params: na x nb cells (each 1..8192, na*nb <= 2^24), the classes that are sources as a bit mask (!= 0),
    max_dist in cells (1..8191), a cell's edge and the inflation radius in map units."""
    _fields_ = [("na", C.c_int), ("nb", C.c_int), ("source_mask", C.c_uint32), ("max_dist", C.c_int), ("cell_size", C.c_double),
                ("inflate_radius", C.c_double)]


class GridClearanceOut(C.Structure):
    """svo_grid_clearance_out: na*nb elements each; every pointer but dist2 may be None."""
    _fields_ = [("dist2", C.c_void_p), ("nearest", C.c_void_p), ("clearance", C.c_void_p), ("blocked", C.c_void_p)]


GRID_CLEARANCE_NONE = 0xFFFFFFFF  # SVO_GRID_CLEARANCE_NONE
GRID_CLEARANCE_COUNTS = ("n_sources", "n_reached", "n_unreached", "n_blocked")


def grid_clearance_default_params(grid, voxel_size):
    """svo_grid_clearance_default_params for a VoxelGridParams and its map's voxel size: the grid's na x nb, cell_size = cell_voxels *
    voxel_size, OBSTACLE cells as the sources, max_dist 64 cells, inflate_radius 0 (not tuned on real data)."""
    p = GridClearanceParams()
    if lib().svo_grid_clearance_default_params(C.byref(grid), C.c_float(voxel_size), C.byref(p)) != 0:
        raise SvoError("svo_grid_clearance_default_params: voxel_size must be finite and > 0, the grid's na, nb and cell_voxels in range")
    return p


def grid_clearance_workspace_bytes(na, nb):
    """svo_grid_clearance_workspace_bytes: 4 * na * nb (no GPU involved); 0 for na or nb < 1."""
    return int(lib().svo_grid_clearance_workspace_bytes(int(na), int(nb)))


def _clearance_params(params, overrides):
    """params and / or its fields as keywords; without params the mask, max_dist and inflate_radius of the defaults, and na, nb and
    cell_size from the keywords (the library refuses what is left at 0)."""
    return _params(lambda: GridClearanceParams(0, 0, 1 << VOXEL_GRID_OBSTACLE, 64, 0.0, 0.0), params, **overrides)


class GridSurfaceParams(C.Structure):
    """svo_grid_surface_params: na x nb cells (each 1..8192, na*nb <= 2^24), the classes that are ground as a bit mask (!= 0), a cell's
    edge in map units, the largest step between edge neighbours (+inf: no rule), the footprint's radius in map units
    ((footprint_radius / cell_size)^2 < 226), the largest relief under it (+inf: no rule) and the least share of it that must be
    ground, in 256ths (0..256, 0: no rule)."""
    _fields_ = [("na", C.c_int), ("nb", C.c_int), ("ground_mask", C.c_uint32), ("cell_size", C.c_double), ("max_step", C.c_double),
                ("footprint_radius", C.c_double), ("max_relief", C.c_double), ("min_support_256", C.c_int)]


class GridSurfaceOut(C.Structure):
    """svo_grid_surface_out: na*nb elements each; every pointer but cls_out may be None; cls_out must not be cls."""
    _fields_ = [("cls_out", C.c_void_p), ("step", C.c_void_p), ("relief", C.c_void_p), ("support", C.c_void_p)]


GRID_SURFACE_STEP, GRID_SURFACE_ROUGH, GRID_SURFACE_UNSUPPORTED = 3, 4, 5
GRID_SURFACE_SOURCES = 1 << 2 | 1 << 3 | 1 << 4 | 1 << 5  # SVO_GRID_SURFACE_SOURCES: the clearance's source_mask over cls_out
GRID_SURFACE_COUNTS = ("n_ground", "n_step", "n_rough", "n_unsupported", "n_nonfinite", "n_kept")


def grid_surface_default_params(grid, voxel_size):
    """svo_grid_surface_default_params for a VoxelGridParams and its map's voxel size: the grid's na x nb, cell_size = cell_voxels *
    voxel_size, LEVEL cells as the ground, max_step = obstacle_step, a footprint of 1.5 cells, max_relief = 2 * obstacle_step,
    min_support_256 0 (not tuned on real data)."""
    p = GridSurfaceParams()
    if lib().svo_grid_surface_default_params(C.byref(grid), C.c_float(voxel_size), C.byref(p)) != 0:
        raise SvoError("svo_grid_surface_default_params: voxel_size must be finite and > 0, the grid's na, nb, cell_voxels and obstacle_step in range")
    return p


def grid_surface_footprint_cells(r2):
    """svo_grid_surface_footprint_cells: the number of offsets (da, db) with da^2 + db^2 <= r2 (no GPU involved); 0 for r2 > 225."""
    return int(lib().svo_grid_surface_footprint_cells(int(r2)))


class GridRouteParams(C.Structure):
    """svo_grid_route_params: na x nb cells (each 1..8192, na*nb <= 2^24), the penalty's squared radius in cells and its weight
    (near_weight * near_r2 <= 2^20), the cap on a cell's cost (1..0x7F000000), the rounds one call enqueues (1..4096), the cells
    written per path (1..2^20, read only with starts) and resume (0 or 1)."""
    _fields_ = [("na", C.c_int), ("nb", C.c_int), ("near_r2", C.c_uint32), ("near_weight", C.c_uint32), ("max_cost", C.c_uint32),
                ("max_rounds", C.c_int), ("max_path", C.c_int), ("resume", C.c_int)]


class GridRouteOut(C.Structure):
    """svo_grid_route_out: cost and next na*nb elements, path n_starts x max_path, path_len and path_status n_starts; every pointer
    but cost may be None, the three of the paths only together."""
    _fields_ = [("cost", C.c_void_p), ("next", C.c_void_p), ("path", C.c_void_p), ("path_len", C.c_void_p), ("path_status", C.c_void_p)]


GRID_ROUTE_NONE = 0xFFFFFFFF  # SVO_GRID_ROUTE_NONE
GRID_ROUTE_MAX_COST = 0x7F000000  # SVO_GRID_ROUTE_MAX_COST
GRID_ROUTE_COUNTS = ("n_goals_used", "n_reached", "n_unreached", "n_impassable", "converged", "rounds_run")
GRID_ROUTE_OK, GRID_ROUTE_TRUNCATED, GRID_ROUTE_UNREACHED, GRID_ROUTE_OUT_OF_GRID, GRID_ROUTE_NOT_CONVERGED = range(5)


def grid_route_default_params(clearance):
    """svo_grid_route_default_params for a GridClearanceParams: its na x nb, no penalty, max_cost 0x7F000000, 64 rounds, paths of up
    to 4096 cells, no resume (not tuned on real data)."""
    p = GridRouteParams()
    if lib().svo_grid_route_default_params(C.byref(clearance), C.byref(p)) != 0:
        raise SvoError("svo_grid_route_default_params: the clearance's na and nb must be in range")
    return p


def grid_route_workspace_bytes(na, nb):
    """svo_grid_route_workspace_bytes (no GPU involved); 0 for na or nb < 1."""
    return int(lib().svo_grid_route_workspace_bytes(int(na), int(nb)))


def _route_params(params, overrides):
    """params and / or its fields as keywords; without params the defaults' penalty, cap, rounds and path length, and na and nb from
    the keywords (the library refuses what is left at 0)."""
    return _params(lambda: GridRouteParams(0, 0, 0, 0, GRID_ROUTE_MAX_COST, 64, 4096, 0), params, **overrides)


class GridFrontierParams(C.Structure):
    """svo_grid_frontier_params: na x nb cells (each 1..8192, na*nb <= 2^24), the classes that are FREE and those that are UNKNOWN as
    bit masks (each != 0, no common bit), the smallest frontier kept in cells (1..2^24) and the records written (1..65536)."""
    _fields_ = [("na", C.c_int), ("nb", C.c_int), ("free_mask", C.c_uint32), ("unknown_mask", C.c_uint32), ("min_size", C.c_uint32),
                ("max_frontiers", C.c_int)]


class GridFrontierOut(C.Structure):
    """svo_grid_frontier_out: frontiers max_frontiers records of GRID_FRONTIER_DTYPE, goal_cells max_frontiers uint32, label na*nb
    uint32; each may be None, but not all three."""
    _fields_ = [("frontiers", C.c_void_p), ("goal_cells", C.c_void_p), ("label", C.c_void_p)]


GRID_FRONTIER_NONE = 0xFFFFFFFF  # SVO_GRID_FRONTIER_NONE
GRID_FRONTIER_COUNTS = ("n_free", "n_unknown", "n_frontier_cells", "n_frontiers", "n_kept", "n_written", "n_kept_cells")
GRID_FRONTIER_COMBINE_DEFAULT = True  # svo_grid_frontier_set_mode's state of a new context
# svo_grid_frontier: 48 bytes
GRID_FRONTIER_DTYPE = np.dtype([("first_cell", "<u4"), ("size", "<u4"), ("rep_cell", "<u4"), ("best_cell", "<u4"), ("best_cost", "<u4"),
                                ("min_a", "<u2"), ("max_a", "<u2"), ("min_b", "<u2"), ("max_b", "<u2"), ("reserved", "<u4"),
                                ("sum_a", "<u8"), ("sum_b", "<u8")])
assert GRID_FRONTIER_DTYPE.itemsize == 48


def grid_frontier_default_params(clearance):
    """svo_grid_frontier_default_params for a GridClearanceParams: its na x nb, LEVEL cells free, UNKNOWN cells unknown, min_size 3,
    max_frontiers 1024 (not tuned on real data)."""
    p = GridFrontierParams()
    if lib().svo_grid_frontier_default_params(C.byref(clearance), C.byref(p)) != 0:
        raise SvoError("svo_grid_frontier_default_params: the clearance's na and nb must be in range")
    return p


def grid_frontier_workspace_bytes(na, nb, max_frontiers):
    """svo_grid_frontier_workspace_bytes (no GPU involved); 0 for a refused shape or max_frontiers."""
    return int(lib().svo_grid_frontier_workspace_bytes(int(na), int(nb), int(max_frontiers)))


def _frontier_params(params, overrides):
    """params and / or its fields as keywords; without params the defaults' masks, min_size and max_frontiers, and na and nb from the
    keywords (the library refuses what is left at 0)."""
    return _params(lambda: GridFrontierParams(0, 0, 1 << VOXEL_GRID_LEVEL, 1 << VOXEL_GRID_UNKNOWN, 3, 1024), params, **overrides)


class GridViewParams(C.Structure):
    """svo_grid_view_params: na x nb cells (each 1..8192, na*nb <= 2^24), the classes that are OPAQUE and those that are GAIN as bit
    masks (each != 0; they may share bits), the range in cells (1..255), the score per visible GAIN cell (1..65536) and what the cost
    is divided by before it is taken off (1..2^31)."""
    _fields_ = [("na", C.c_int), ("nb", C.c_int), ("opaque_mask", C.c_uint32), ("gain_mask", C.c_uint32), ("max_range", C.c_int),
                ("gain_weight", C.c_uint32), ("cost_div", C.c_uint32)]


class GridViewOut(C.Structure):
    """svo_grid_view_out: records n_views records of GRID_VIEW_DTYPE, order n_views uint32, best 4 uint32, seen na*nb uint32; each may
    be None, but not all four."""
    _fields_ = [("records", C.c_void_p), ("order", C.c_void_p), ("best", C.c_void_p), ("seen", C.c_void_p)]


GRID_VIEW_NONE = 0xFFFFFFFF  # SVO_GRID_VIEW_NONE
GRID_VIEW_MAX_VIEWS = 4096  # SVO_GRID_VIEW_MAX_VIEWS
GRID_VIEW_COUNTS = ("n_used", "n_ignored", "n_in_range", "n_visible", "n_gain", "n_covered", "n_gain_covered")
GRID_VIEW_BEST = ("cell", "index", "score", "n_gain")
GRID_VIEW_STAGED_DEFAULT = True  # svo_grid_view_set_mode's state of a new context
# svo_grid_view_rec: 32 bytes
GRID_VIEW_DTYPE = np.dtype([("cell", "<u4"), ("n_visible", "<u4"), ("n_gain", "<u4"), ("n_opaque", "<u4"), ("cost", "<u4"), ("score", "<u4"),
                            ("reserved", "<u4", (2,))])
assert GRID_VIEW_DTYPE.itemsize == 32


def grid_view_default_params(clearance):
    """svo_grid_view_default_params for a GridClearanceParams: its na x nb, OBSTACLE cells opaque, UNKNOWN cells the gain, max_range
    min(its max_dist, 255), gain_weight 16, cost_div 1 (not tuned on real data)."""
    p = GridViewParams()
    if lib().svo_grid_view_default_params(C.byref(clearance), C.byref(p)) != 0:
        raise SvoError("svo_grid_view_default_params: the clearance's na and nb must be in range")
    return p


def grid_view_workspace_bytes(na, nb, n_views):
    """svo_grid_view_workspace_bytes (no GPU involved); 0 for a refused shape or n_views."""
    return int(lib().svo_grid_view_workspace_bytes(int(na), int(nb), int(n_views)))


def _view_params(params, overrides):
    """params and / or its fields as keywords; without params the defaults' masks, range 64, weight and divisor, and na and nb from the
    keywords (the library refuses what is left at 0)."""
    return _params(lambda: GridViewParams(0, 0, 1 << VOXEL_GRID_OBSTACLE, 1 << VOXEL_GRID_UNKNOWN, 64, 16, 1), params, **overrides)


class GridWaypointParams(C.Structure):
    """svo_grid_waypoint_params: na x nb cells (each 1..8192, na*nb <= 2^24), the entries between two rows of path (the route's
    max_path, 1..2^20), the longest segment in cells and in path entries (1..255), the squared distance in cells below which a cell
    with a dist2 is SOLID (0..2^26; 0: none), the waypoints written per path (1..2^20) and a cell's edge in map units (finite, > 0)."""
    _fields_ = [("na", C.c_int), ("nb", C.c_int), ("path_stride", C.c_int), ("max_look", C.c_int), ("min_dist2", C.c_uint32),
                ("max_way", C.c_int), ("cell_size", C.c_double)]


class GridWaypointOut(C.Structure):
    """svo_grid_waypoint_out: way and way_index n_paths * max_way uint32, way_len n_paths uint32, way_status n_paths uint8, length
    n_paths float64; each may be None, but not all, and way and way_len only together."""
    _fields_ = [("way", C.c_void_p), ("way_index", C.c_void_p), ("way_len", C.c_void_p), ("way_status", C.c_void_p), ("length", C.c_void_p)]


GRID_WAY_NONE = 0xFFFFFFFF  # what grid_waypoints_host fills way and way_index with before the call
GRID_WAY_MAX_PATHS = 4096  # SVO_GRID_WAY_MAX_PATHS
GRID_WAY_OK, GRID_WAY_PATH_TRUNCATED, GRID_WAY_FULL, GRID_WAY_SKIPPED, GRID_WAY_BAD_CELL = 0, 1, 2, 4, 5  # SVO_GRID_WAY_*
GRID_WAY_COUNTS = ("n_used", "n_skipped", "n_cells_in", "n_waypoints", "n_forced", "n_full", "max_d2")


def grid_waypoints_default_params(route_params, clearance_params):
    """svo_grid_waypoints_default_params for a GridRouteParams and the GridClearanceParams it read: the route's na x nb, path_stride
    = its max_path, max_look 64, min_dist2 0, max_way 256, the clearance's cell_size (not tuned on real data)."""
    p = GridWaypointParams()
    if lib().svo_grid_waypoints_default_params(C.byref(route_params), C.byref(clearance_params), C.byref(p)) != 0:
        raise SvoError("svo_grid_waypoints_default_params: the route's na, nb and max_path and the clearance's cell_size must be in range")
    return p


SPECKLE_TILE = (64, 16)  # SVO_SPECKLE_TILE_W, SVO_SPECKLE_TILE_H


def speckle_workspace_bytes(width, height, batch=1):
    """svo_speckle_workspace_bytes: device bytes the batched speckle filter needs (no GPU involved)."""
    return int(lib().svo_speckle_workspace_bytes(width, height, batch))


CLOUD_POINT_DTYPE = np.dtype([("x", np.float32), ("y", np.float32), ("z", np.float32), ("tag", np.uint32)])


class KeyframeCloud(C.Structure):
    """svo_keyframe_cloud: one entry of a pipeline's / group's table of the last process call."""
    _fields_ = [("frame", C.c_int), ("lane", C.c_int), ("n_total", C.c_int), ("n_stored", C.c_int), ("dev", C.c_void_p)]


def cloud_default_params(width, height):
    """svo_cloud_default_params: step 1, min_disparity 0, max_points width*height."""
    p = CloudParams()
    if lib().svo_cloud_default_params(C.byref(p), width, height) != 0:
        raise SvoError("svo_cloud_default_params failed")
    return p


def _cloud_params(width, height, step, min_disparity, max_points):
    return CloudParams(int(step), float(min_disparity), int(width * height if max_points is None else max_points))


def _keyframe_disparity(ctx, h, fn, i):
    """Entry i's device map pointer (an int) of the last process call."""
    dev = C.c_void_p()
    ctx._chk(fn(h, int(i), C.byref(dev)), fn.__name__)
    return dev.value


def _keyframe_disparity_host(ctx, h, fn, i, width, height):
    d = np.empty((height, width), np.int16)
    ctx._chk(fn(h, int(i), _p(d)), fn.__name__)
    return d


def _keyframe_clouds(ctx, L, h, table_fn, copy_fn):
    """The table of the last process call as a list of dicts; "points": numpy structured array (CLOUD_POINT_DTYPE) of n_stored records."""
    n, tab = C.c_int(0), C.POINTER(KeyframeCloud)()
    ctx._chk(table_fn(h, C.byref(n), C.byref(tab)), table_fn.__name__)
    out = []
    for i in range(n.value):
        e = tab[i]
        pts = np.empty(e.n_stored, CLOUD_POINT_DTYPE)
        ctx._chk(copy_fn(h, i, _p(pts), e.n_stored), copy_fn.__name__)
        out.append({"frame": e.frame, "lane": e.lane, "n_total": e.n_total, "n_stored": e.n_stored, "dev": e.dev, "points": pts})
    return out


class SynthParams(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("width", C.c_int), ("height", C.c_int), ("focal", C.c_double),
                ("cx", C.c_double), ("cy", C.c_double), ("baseline", C.c_double), ("step_z", C.c_double),
                ("step_x", C.c_double), ("yaw_per_frame", C.c_double), ("n_billboards", C.c_int)]


REFERENCE_CONSTANT_NAMES = (
    "gftt_max_corners", "gftt_quality", "min_detected", "keyframe_percent_lost", "pnp_iterations", "pnp_reproj_error",
    "pnp_confidence", "stereo_num_disparities", "stereo_block_size", "stereo_disparity_scale",
    "triangulate_min_disparity_exclusive", "lk_win_w", "lk_win_h", "lk_max_level", "lk_max_iterations", "lk_epsilon",
    "lk_min_eig_threshold", "fb_max_distance", "max_parallax", "draw_thickness", "parallax_thresh", "min_feature_distance",
    "sliding_window_size", "max_features", "ba_max_solver_time_s", "ba_num_threads")


class ReferenceConstants(C.Structure):
    _fields_ = [(n, C.c_double) for n in REFERENCE_CONSTANT_NAMES]


def reference_constants():
    """The reference's first-party literals as compiled into the library (svo_reference_constants)."""
    c = ReferenceConstants()
    if lib().svo_reference_constants(C.byref(c)) != 0:
        raise SvoError("svo_reference_constants failed")
    return {n: getattr(c, n) for n in REFERENCE_CONSTANT_NAMES}


class LmStats(C.Structure):
    _fields_ = [("linearize_calls", C.c_int), ("step_calls", C.c_int), ("speculations", C.c_int), ("speculation_hits", C.c_int),
                ("single_exchange", C.c_int), ("collectives", C.c_int), ("device_control", C.c_int), ("fallbacks", C.c_int),
                ("host_us", C.c_double)]


class LmStepCtl(C.Structure):
    _fields_ = [("cost", C.c_double), ("mcc", C.c_double), ("decrease_factor", C.c_double), ("spec_radius", C.c_double),
                ("chain", C.c_int)]


LM_LINEARIZE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_double, C.c_int, C.POINTER(C.c_double))
LM_STEP_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double, C.POINTER(LmStepCtl),
                         C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int))
LM_ACCEPT_FN = C.CFUNCTYPE(C.c_int, C.c_void_p)


class LmOps(C.Structure):
    _fields_ = [("user", C.c_void_p), ("linearize", LM_LINEARIZE_FN), ("step", LM_STEP_FN), ("accept", LM_ACCEPT_FN)]


def lm_decide_step(cost, mcc, radius, decrease_factor, cost_new, model_change_points):
    """svo_lm_decide_step: Ceres' accept / radius rule -> (accept, next_radius)."""
    acc, rad = C.c_int(0), C.c_double(0.0)
    lib().svo_lm_decide_step(C.c_double(cost), C.c_double(mcc), C.c_double(radius), C.c_double(decrease_factor), C.c_double(cost_new),
                             C.c_double(model_change_points), C.byref(acc), C.byref(rad))
    return bool(acc.value), rad.value


def lm_solve(poses7, linearize, step, accept, max_iterations=50, max_time_s=0.0):
    """svo_lm_solve — the product's LM step control (host/lm.cpp) over caller-provided passes (no GPU involved).
    linearize(radius, first) -> payload1 array;
    step(dc, cand_poses, radius, ctl) -> (payload2, payload1_next or None, next_radius, next_at_candidate) with ctl an
    LmStepCtl (cost, mcc, decrease_factor, spec_radius, chain);  accept() -> None.
    Returns (poses7, BASummary, LmStats)."""
    poses = np.ascontiguousarray(poses7, np.float64).copy()
    K = poses.shape[0]
    n = 6 * (K - 1)
    pay1 = n * n + 3 * n + 2

    def _lin(user, radius, first, out):
        np.ctypeslib.as_array(out, shape=(pay1,))[:] = linearize(radius, first)
        return 0

    def _step(user, dc, cand, radius, ctl, out2, out1, out_radius, out_at_cand):
        d = np.ctypeslib.as_array(dc, shape=(max(n, 1),))[:n].copy()
        c = np.ctypeslib.as_array(cand, shape=(K, 7)).copy()
        p2, p1, nr, at_cand = step(d, c, radius, ctl.contents)
        np.ctypeslib.as_array(out2, shape=(4,))[:] = p2
        if p1 is not None:
            np.ctypeslib.as_array(out1, shape=(pay1,))[:] = p1
        out_radius[0] = nr if p1 is not None else 0.0
        out_at_cand[0] = int(bool(at_cand))
        return 0

    def _acc(user):
        accept()
        return 0
    ops = LmOps(None, LM_LINEARIZE_FN(_lin), LM_STEP_FN(_step), LM_ACCEPT_FN(_acc))
    opt = ba_default_options()
    opt.max_iterations, opt.max_time_s = max_iterations, max_time_s
    s, st = BASummary(), LmStats()
    rc = lib().svo_lm_solve(K, _p(poses), C.byref(ops), C.byref(opt), C.byref(s), C.byref(st))
    if rc:
        raise SvoError(f"svo_lm_solve failed ({rc})")
    return poses, s, st


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_size_t, C.c_void_p)

# every symbol include/svo.h declares (tests check that the library exports all of them)
SYMBOLS = [
    "svo_create", "svo_destroy", "svo_last_error", "svo_stream", "svo_sync", "svo_version", "svo_reference_constants",
    "svo_profile_select", "svo_profile_read", "svo_measure_peak",
    "svo_reproj_eval", "svo_reproj_eval_dev",
    "svo_corner_detect", "svo_corner_detect_batch_dev", "svo_corner_response",
    "svo_stereo_bm", "svo_stereo_disparity_at", "svo_stereo_disparity_at_dev",
    "svo_triangulate", "svo_lk_track", "svo_build_pyramid", "svo_track_features", "svo_dedup",
    "svo_pnp_ransac",
    "svo_ba_default_options", "svo_ba_create", "svo_ba_destroy", "svo_ba_reset", "svo_ba_add_keyframe", "svo_ba_solve",
    "svo_ba_get_pose", "svo_ba_window_count", "svo_ba_get_points", "svo_ba_load_problem",
    "svo_ba_set_allreduce", "svo_ba_set_device_lm", "svo_ba_set_bulk_control", "svo_ba_set_solve_form", "svo_ba_wave_chunks_limit", "svo_ba_set_wave_chunks", "svo_ba_set_yield_iterations", "svo_ba_solve_forms", "svo_ba_solve_problem", "svo_ba_solve_problems", "svo_ba_read_problem", "svo_ba_set_comm", "svo_ba_last_stats", "svo_lm_solve", "svo_lm_decide_step",
    "svo_rccl_unique_id", "svo_rccl_comm_create", "svo_rccl_comm_destroy",
    "svo_pipeline_default_params", "svo_pipeline_create", "svo_pipeline_destroy", "svo_pipeline_reset",
    "svo_pipeline_process_batch_dev", "svo_pipeline_process_batch", "svo_pipeline_get_tracked",
    "svo_pipeline_group_create", "svo_pipeline_group_destroy", "svo_pipeline_group_reset", "svo_pipeline_group_lanes",
    "svo_pipeline_group_process_batch_dev", "svo_pipeline_group_get_tracked", "svo_pipeline_group_last_stats",
    "svo_pipeline_group_solve_work", "svo_pipeline_group_solve_forms", "svo_pipeline_group_set_solve_yield", "svo_pipeline_group_staging", "svo_pipeline_group_upload", "svo_pipeline_group_process_uploaded", "svo_pipeline_group_process_batch",
    "svo_synth_default_params", "svo_synth_render", "svo_synth_pose",
    "svo_image_read_gray", "svo_kitti_read_poses", "svo_ate_rmse", "svo_kitti_run", "svo_cholesky_solve", "svo_cholesky_solve_dev", "svo_draw_track", "svo_pipeline_draw_track",
    "svo_rectify_eye_from_camera_info", "svo_rectify_build_map", "svo_rectify_remap", "svo_rectify_remap_batch_dev",
    "svo_pipeline_set_rectification", "svo_pipeline_group_set_rectification",
    "svo_stereo_bm_batch_dev", "svo_cloud_default_params", "svo_disparity_cloud_batch_dev", "svo_stereo_cloud",
    "svo_pipeline_set_keyframe_clouds", "svo_pipeline_keyframe_clouds", "svo_pipeline_copy_keyframe_cloud",
    "svo_pipeline_group_set_keyframe_clouds", "svo_pipeline_group_keyframe_clouds", "svo_pipeline_group_copy_keyframe_cloud",
    "svo_speckle_workspace_bytes", "svo_disparity_speckle_filter_batch_dev", "svo_disparity_speckle_filter",
    "svo_pipeline_set_keyframe_speckle_filter", "svo_pipeline_group_set_keyframe_speckle_filter",
    "svo_stereo_bm_cost_batch_dev", "svo_disparity_lr_check_batch_dev", "svo_disparity_lr_check",
    "svo_pipeline_set_keyframe_lr_check", "svo_pipeline_group_set_keyframe_lr_check",
    "svo_sgm_default_params", "svo_sgm_workspace_bytes", "svo_stereo_sgm_batch_dev", "svo_stereo_sgm",
    "svo_pipeline_set_keyframe_sgm", "svo_pipeline_group_set_keyframe_sgm",
    "svo_voxel_map_default_params", "svo_voxel_map_bytes", "svo_voxel_map_create", "svo_voxel_map_destroy", "svo_voxel_map_clear",
    "svo_voxel_map_insert_dev", "svo_pose7_to_cam_to_world", "svo_voxel_map_insert_pose7_dev", "svo_voxel_map_stats",
    "svo_voxel_map_extract_dev", "svo_voxel_map_extract", "svo_voxel_map_download",
    "svo_voxel_carve_default_params", "svo_voxel_map_carve_dev", "svo_pose7_to_world_to_cam", "svo_voxel_map_carve_pose7_dev",
    "svo_voxel_map_carve", "svo_voxel_map_copy_live_dev", "svo_pipeline_keyframe_disparity", "svo_pipeline_group_keyframe_disparity",
    "svo_pipeline_copy_keyframe_disparity", "svo_pipeline_group_copy_keyframe_disparity",
    "svo_voxel_render_default_params", "svo_voxel_render_workspace_bytes", "svo_voxel_map_render_dev", "svo_voxel_map_render_pose7_dev",
    "svo_voxel_map_render", "svo_voxel_render_set_mode",
    "svo_voxel_grid_default_params", "svo_voxel_grid_workspace_bytes", "svo_voxel_grid_cell_of", "svo_voxel_map_grid_dev", "svo_voxel_map_grid",
    "svo_voxel_grid_set_mode",
    "svo_grid_surface_default_params", "svo_grid_surface_footprint_cells", "svo_grid_surface_dev", "svo_grid_surface",
    "svo_grid_clearance_default_params", "svo_grid_clearance_workspace_bytes", "svo_grid_clearance_dev", "svo_grid_clearance",
    "svo_grid_route_default_params", "svo_grid_route_workspace_bytes", "svo_grid_route_dev", "svo_grid_route",
    "svo_grid_frontier_default_params", "svo_grid_frontier_workspace_bytes", "svo_grid_frontiers_dev", "svo_grid_frontiers",
    "svo_grid_frontier_set_mode",
    "svo_grid_view_default_params", "svo_grid_view_workspace_bytes", "svo_grid_view_dev", "svo_grid_view", "svo_grid_view_set_mode",
    "svo_grid_waypoints_default_params", "svo_grid_waypoints_dev", "svo_grid_waypoints",
    "svo_voxel_map_remove_dev", "svo_voxel_map_remove_pose7_dev", "svo_voxel_map_remove_sync", "svo_voxel_map_move_dev", "svo_voxel_map_move_pose7_dev",
    "svo_voxel_ledger_bytes", "svo_voxel_ledger_create", "svo_voxel_ledger_destroy", "svo_voxel_ledger_insert_pose7_dev",
    "svo_voxel_ledger_update_pose7", "svo_voxel_ledger_retire", "svo_voxel_ledger_remove", "svo_voxel_ledger_ids", "svo_voxel_ledger_get",
    "svo_voxel_align_default_params", "svo_voxel_map_align_sums_dev", "svo_voxel_map_align_sums_pose7_dev", "svo_voxel_map_align",
    "svo_voxel_normals_default_params", "svo_voxel_map_normals_bytes", "svo_voxel_map_normals_dev", "svo_voxel_map_normals",
    "svo_voxel_map_align_plane_sums_dev", "svo_voxel_map_align_plane_sums_pose7_dev", "svo_voxel_map_align_plane",
    "svo_voxel_occupancy_bytes", "svo_voxel_map_occupancy_dev", "svo_voxel_map_occupancy", "svo_voxel_map_locate_scores_dev",
    "svo_voxel_locate_default_params", "svo_voxel_locate_workspace_bytes", "svo_voxel_map_locate",
    "svo_voxel_raycast_default_params", "svo_voxel_occupancy_coarse_bytes", "svo_voxel_occupancy_coarse_dev", "svo_voxel_occupancy_rays_dev",
    "svo_voxel_occupancy_rays", "svo_voxel_occupancy_raycast_dev", "svo_voxel_occupancy_raycast_pose7_dev", "svo_voxel_map_raycast",
    "svo_voxel_distance_default_params", "svo_voxel_distance_workspace_bytes", "svo_voxel_distance_bytes", "svo_voxel_occupancy_distance_dev",
    "svo_voxel_distance_query_dev", "svo_voxel_distance_query", "svo_voxel_map_distance",
    "svo_voxel_route_default_params", "svo_voxel_route_workspace_bytes", "svo_voxel_occupancy_cell_of", "svo_voxel_occupancy_route_dev",
    "svo_voxel_occupancy_route",
]


def lib():
    """Load libsvo_hip.so (raises if it has not been built: there is no fallback)."""
    global _LIB
    if _LIB is None:
        p = lib_path()
        if not os.path.exists(p):
            raise SvoError(f"{p} not built — run `python -c 'import __graft_entry__ as g; g.build()'`")
        L = C.CDLL(p)
        L.svo_version.restype = C.c_char_p
        L.svo_last_error.restype = C.c_char_p
        L.svo_last_error.argtypes = [C.c_void_p]
        L.svo_stream.restype = C.c_void_p
        L.svo_stream.argtypes = [C.c_void_p]
        L.svo_destroy.argtypes = [C.c_void_p]
        L.svo_destroy.restype = None
        # dense depth clouds: every entry with its full signature (pointers and size_t do not survive ctypes' int default)
        vp, ci, sz = C.c_void_p, C.c_int, C.c_size_t
        L.svo_cloud_default_params.argtypes = [vp, ci, ci]
        L.svo_stereo_bm_batch_dev.argtypes = [vp, vp, vp, ci, ci, ci, ci, sz, ci, ci, vp]
        L.svo_disparity_cloud_batch_dev.argtypes = [vp, vp, vp, ci, ci, ci, ci, sz, vp, vp, vp, vp, vp]
        L.svo_stereo_cloud.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp]
        L.svo_pipeline_set_keyframe_clouds.argtypes = [vp, vp, ci]
        L.svo_pipeline_keyframe_clouds.argtypes = [vp, vp, vp]
        L.svo_pipeline_copy_keyframe_cloud.argtypes = [vp, ci, vp, ci]
        L.svo_pipeline_group_set_keyframe_clouds.argtypes = [vp, ci, vp, ci]
        L.svo_pipeline_group_keyframe_clouds.argtypes = [vp, vp, vp]
        L.svo_pipeline_group_copy_keyframe_cloud.argtypes = [vp, ci, vp, ci]
        for f in ("svo_cloud_default_params", "svo_stereo_bm_batch_dev", "svo_disparity_cloud_batch_dev", "svo_stereo_cloud",
                  "svo_pipeline_set_keyframe_clouds", "svo_pipeline_keyframe_clouds", "svo_pipeline_copy_keyframe_cloud",
                  "svo_pipeline_group_set_keyframe_clouds", "svo_pipeline_group_keyframe_clouds", "svo_pipeline_group_copy_keyframe_cloud"):
            getattr(L, f).restype = ci
        # speckle filter
        L.svo_speckle_workspace_bytes.argtypes = [ci, ci, ci]
        L.svo_speckle_workspace_bytes.restype = sz
        L.svo_disparity_speckle_filter_batch_dev.argtypes = [vp, vp, ci, ci, ci, vp, vp, sz, vp]
        L.svo_disparity_speckle_filter.argtypes = [vp, vp, ci, ci, vp, vp]
        L.svo_pipeline_set_keyframe_speckle_filter.argtypes = [vp, vp]
        L.svo_pipeline_group_set_keyframe_speckle_filter.argtypes = [vp, vp]
        for f in ("svo_disparity_speckle_filter_batch_dev", "svo_disparity_speckle_filter", "svo_pipeline_set_keyframe_speckle_filter",
                  "svo_pipeline_group_set_keyframe_speckle_filter"):
            getattr(L, f).restype = ci
        # left-right check
        L.svo_stereo_bm_cost_batch_dev.argtypes = [vp, vp, vp, ci, ci, ci, ci, sz, ci, ci, vp, vp]
        L.svo_disparity_lr_check_batch_dev.argtypes = [vp, vp, vp, ci, ci, ci, vp, vp]
        L.svo_disparity_lr_check.argtypes = [vp, vp, vp, ci, ci, vp, vp]
        L.svo_pipeline_set_keyframe_lr_check.argtypes = [vp, vp]
        L.svo_pipeline_group_set_keyframe_lr_check.argtypes = [vp, vp]
        for f in ("svo_stereo_bm_cost_batch_dev", "svo_disparity_lr_check_batch_dev", "svo_disparity_lr_check",
                  "svo_pipeline_set_keyframe_lr_check", "svo_pipeline_group_set_keyframe_lr_check"):
            getattr(L, f).restype = ci
        # semi-global matching
        L.svo_sgm_default_params.argtypes = [vp, ci]
        L.svo_sgm_workspace_bytes.argtypes = [ci, ci, ci, ci, ci]
        L.svo_sgm_workspace_bytes.restype = sz
        L.svo_stereo_sgm_batch_dev.argtypes = [vp, vp, vp, ci, ci, ci, ci, sz, ci, ci, vp, vp, sz, vp, vp]
        L.svo_stereo_sgm.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, vp, vp, vp]
        L.svo_pipeline_set_keyframe_sgm.argtypes = [vp, vp]
        L.svo_pipeline_group_set_keyframe_sgm.argtypes = [vp, vp]
        for f in ("svo_sgm_default_params", "svo_stereo_sgm_batch_dev", "svo_stereo_sgm", "svo_pipeline_set_keyframe_sgm",
                  "svo_pipeline_group_set_keyframe_sgm"):
            getattr(L, f).restype = ci
        # voxel map
        L.svo_voxel_map_default_params.argtypes = [vp]
        L.svo_voxel_map_bytes.argtypes = [vp, vp]
        L.svo_voxel_map_create.argtypes = [vp, vp, vp]
        L.svo_voxel_map_destroy.argtypes = [vp]
        L.svo_voxel_map_destroy.restype = None
        L.svo_voxel_map_clear.argtypes = [vp]
        L.svo_voxel_map_insert_dev.argtypes = [vp, vp, ci, vp]
        L.svo_pose7_to_cam_to_world.argtypes = [vp, vp]
        L.svo_voxel_map_insert_pose7_dev.argtypes = [vp, vp, ci, vp]
        L.svo_voxel_map_stats.argtypes = [vp, vp]
        L.svo_voxel_map_extract_dev.argtypes = [vp, ci, vp, ci, vp]
        L.svo_voxel_map_extract.argtypes = [vp, ci, vp, ci, vp, vp]
        L.svo_voxel_map_download.argtypes = [vp, vp, sz]
        for f in ("svo_voxel_map_default_params", "svo_voxel_map_bytes", "svo_voxel_map_create", "svo_voxel_map_clear",
                  "svo_voxel_map_insert_dev", "svo_pose7_to_cam_to_world", "svo_voxel_map_insert_pose7_dev", "svo_voxel_map_stats",
                  "svo_voxel_map_extract_dev", "svo_voxel_map_extract", "svo_voxel_map_download"):
            getattr(L, f).restype = ci
        # carving and the copy of the live voxels
        L.svo_voxel_carve_default_params.argtypes = [vp]
        L.svo_voxel_map_carve_dev.argtypes = [vp, vp, ci, ci, vp, vp, vp, vp]
        L.svo_pose7_to_world_to_cam.argtypes = [vp, vp]
        L.svo_voxel_map_carve_pose7_dev.argtypes = [vp, vp, ci, ci, vp, vp, vp, vp]
        L.svo_voxel_map_carve.argtypes = [vp, vp, ci, ci, vp, vp, vp, vp]
        L.svo_voxel_map_copy_live_dev.argtypes = [vp, vp, ci, vp]
        L.svo_pipeline_keyframe_disparity.argtypes = [vp, ci, vp]
        L.svo_pipeline_group_keyframe_disparity.argtypes = [vp, ci, vp]
        L.svo_pipeline_copy_keyframe_disparity.argtypes = [vp, ci, vp]
        L.svo_pipeline_group_copy_keyframe_disparity.argtypes = [vp, ci, vp]
        for f in ("svo_voxel_carve_default_params", "svo_voxel_map_carve_dev", "svo_pose7_to_world_to_cam", "svo_voxel_map_carve_pose7_dev",
                  "svo_voxel_map_carve", "svo_voxel_map_copy_live_dev", "svo_pipeline_keyframe_disparity",
                  "svo_pipeline_group_keyframe_disparity", "svo_pipeline_copy_keyframe_disparity",
                  "svo_pipeline_group_copy_keyframe_disparity"):
            getattr(L, f).restype = ci
        # the render
        L.svo_voxel_render_default_params.argtypes = [vp]
        L.svo_voxel_render_workspace_bytes.argtypes = [ci, ci]
        L.svo_voxel_render_workspace_bytes.restype = sz
        L.svo_voxel_map_render_dev.argtypes = [vp, ci, ci, vp, vp, vp, vp, vp, vp, vp]
        L.svo_voxel_map_render_pose7_dev.argtypes = [vp, ci, ci, vp, vp, vp, vp, vp, vp, vp]
        L.svo_voxel_map_render.argtypes = [vp, ci, ci, vp, vp, vp, vp, vp, vp]
        L.svo_voxel_render_set_mode.argtypes = [vp, ci, ci]
        for f in ("svo_voxel_render_default_params", "svo_voxel_map_render_dev", "svo_voxel_map_render_pose7_dev", "svo_voxel_map_render",
                  "svo_voxel_render_set_mode"):
            getattr(L, f).restype = ci
        # the grid
        L.svo_voxel_grid_default_params.argtypes = [C.c_float, vp]
        L.svo_voxel_grid_workspace_bytes.argtypes = [ci, ci]
        L.svo_voxel_grid_workspace_bytes.restype = sz
        L.svo_voxel_grid_cell_of.argtypes = [vp, C.c_float, C.c_double, C.c_double, vp, vp]
        L.svo_voxel_map_grid_dev.argtypes = [vp, vp, vp, vp, vp]
        L.svo_voxel_map_grid.argtypes = [vp, vp, vp, vp]
        L.svo_voxel_grid_set_mode.argtypes = [vp, ci]
        for f in ("svo_voxel_grid_default_params", "svo_voxel_grid_cell_of", "svo_voxel_map_grid_dev", "svo_voxel_map_grid", "svo_voxel_grid_set_mode"):
            getattr(L, f).restype = ci
        # the ground plan surface
        L.svo_grid_surface_default_params.argtypes = [vp, C.c_float, vp]
        L.svo_grid_surface_footprint_cells.argtypes = [C.c_uint32]
        L.svo_grid_surface_footprint_cells.restype = C.c_uint32
        L.svo_grid_surface_dev.argtypes = [vp, vp, vp, vp, vp, vp]
        L.svo_grid_surface.argtypes = [vp, vp, vp, vp, vp, vp]
        for f in ("svo_grid_surface_default_params", "svo_grid_surface_dev", "svo_grid_surface"):
            getattr(L, f).restype = ci
        # the ground plan clearance
        L.svo_grid_clearance_default_params.argtypes = [vp, C.c_float, vp]
        L.svo_grid_clearance_workspace_bytes.argtypes = [ci, ci]
        L.svo_grid_clearance_workspace_bytes.restype = sz
        L.svo_grid_clearance_dev.argtypes = [vp, vp, vp, vp, vp, vp]
        L.svo_grid_clearance.argtypes = [vp, vp, vp, vp, vp]
        for f in ("svo_grid_clearance_default_params", "svo_grid_clearance_dev", "svo_grid_clearance"):
            getattr(L, f).restype = ci
        # the ground plan route
        L.svo_grid_route_default_params.argtypes = [vp, vp]
        L.svo_grid_route_workspace_bytes.argtypes = [ci, ci]
        L.svo_grid_route_workspace_bytes.restype = sz
        L.svo_grid_route_dev.argtypes = [vp, vp, vp, vp, vp, ci, vp, ci, vp, vp, vp]
        L.svo_grid_route.argtypes = [vp, vp, vp, vp, vp, ci, vp, ci, vp, vp]
        for f in ("svo_grid_route_default_params", "svo_grid_route_dev", "svo_grid_route"):
            getattr(L, f).restype = ci
        # the ground plan frontiers
        L.svo_grid_frontier_default_params.argtypes = [vp, vp]
        L.svo_grid_frontier_workspace_bytes.argtypes = [ci, ci, ci]
        L.svo_grid_frontier_workspace_bytes.restype = sz
        L.svo_grid_frontiers_dev.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp]
        L.svo_grid_frontiers.argtypes = [vp, vp, vp, vp, vp, vp, vp]
        L.svo_grid_frontier_set_mode.argtypes = [vp, ci]
        for f in ("svo_grid_frontier_default_params", "svo_grid_frontiers_dev", "svo_grid_frontiers", "svo_grid_frontier_set_mode"):
            getattr(L, f).restype = ci
        # the ground plan view
        L.svo_grid_view_default_params.argtypes = [vp, vp]
        L.svo_grid_view_workspace_bytes.argtypes = [ci, ci, ci]
        L.svo_grid_view_workspace_bytes.restype = sz
        L.svo_grid_view_dev.argtypes = [vp, vp, vp, ci, vp, vp, vp, vp, vp]
        L.svo_grid_view.argtypes = [vp, vp, vp, ci, vp, vp, vp, vp]
        L.svo_grid_view_set_mode.argtypes = [vp, ci]
        L.svo_grid_waypoints_default_params.argtypes = [vp, vp, vp]
        L.svo_grid_waypoints_dev.argtypes = [vp, vp, vp, vp, vp, vp, ci, vp, vp, vp]
        L.svo_grid_waypoints.argtypes = [vp, vp, vp, vp, vp, vp, ci, vp, vp, vp]
        for f in ("svo_grid_waypoints_default_params", "svo_grid_waypoints_dev", "svo_grid_waypoints"):
            getattr(L, f).restype = ci
        for f in ("svo_grid_view_default_params", "svo_grid_view_dev", "svo_grid_view", "svo_grid_view_set_mode"):
            getattr(L, f).restype = ci
        # removal, move and the keyframe ledger
        i64 = C.c_int64
        L.svo_voxel_map_remove_dev.argtypes = [vp, vp, ci, vp, vp]
        L.svo_voxel_map_remove_pose7_dev.argtypes = [vp, vp, ci, vp, vp]
        L.svo_voxel_map_remove_sync.argtypes = [vp, vp, ci, vp, vp]
        L.svo_voxel_map_move_dev.argtypes = [vp, vp, ci, vp, vp, vp]
        L.svo_voxel_map_move_pose7_dev.argtypes = [vp, vp, ci, vp, vp, vp]
        L.svo_voxel_ledger_bytes.argtypes = [vp, vp]
        L.svo_voxel_ledger_create.argtypes = [vp, vp, vp]
        L.svo_voxel_ledger_destroy.argtypes = [vp]
        L.svo_voxel_ledger_destroy.restype = None
        L.svo_voxel_ledger_insert_pose7_dev.argtypes = [vp, i64, vp, ci, vp]
        L.svo_voxel_ledger_update_pose7.argtypes = [vp, i64, vp, vp]
        L.svo_voxel_ledger_retire.argtypes = [vp, i64]
        L.svo_voxel_ledger_remove.argtypes = [vp, i64, vp]
        L.svo_voxel_ledger_ids.argtypes = [vp, vp, ci, vp]
        L.svo_voxel_ledger_get.argtypes = [vp, i64, vp, vp, vp]
        for f in ("svo_voxel_map_remove_dev", "svo_voxel_map_remove_pose7_dev", "svo_voxel_map_remove_sync", "svo_voxel_map_move_dev", "svo_voxel_map_move_pose7_dev",
                  "svo_voxel_ledger_bytes", "svo_voxel_ledger_create", "svo_voxel_ledger_insert_pose7_dev", "svo_voxel_ledger_update_pose7",
                  "svo_voxel_ledger_retire", "svo_voxel_ledger_remove", "svo_voxel_ledger_ids", "svo_voxel_ledger_get"):
            getattr(L, f).restype = ci
        # the align
        L.svo_voxel_align_default_params.argtypes = [C.c_float, vp]
        L.svo_voxel_map_align_sums_dev.argtypes = [vp, vp, ci, vp, vp, vp]
        L.svo_voxel_map_align_sums_pose7_dev.argtypes = [vp, vp, ci, vp, vp, vp]
        L.svo_voxel_map_align.argtypes = [vp, vp, ci, vp, vp, vp, vp]
        for f in ("svo_voxel_align_default_params", "svo_voxel_map_align_sums_dev", "svo_voxel_map_align_sums_pose7_dev", "svo_voxel_map_align"):
            getattr(L, f).restype = ci
        # the normals and the plane form of the align
        L.svo_voxel_normals_default_params.argtypes = [vp]
        L.svo_voxel_map_normals_bytes.argtypes = [vp, vp]
        L.svo_voxel_map_normals_dev.argtypes = [vp, vp, vp, vp]
        L.svo_voxel_map_normals.argtypes = [vp, vp, vp, vp]
        L.svo_voxel_map_align_plane_sums_dev.argtypes = [vp, vp, vp, ci, vp, vp, vp]
        L.svo_voxel_map_align_plane_sums_pose7_dev.argtypes = [vp, vp, vp, ci, vp, vp, vp]
        L.svo_voxel_map_align_plane.argtypes = [vp, vp, vp, ci, vp, vp, vp, vp]
        for f in ("svo_voxel_normals_default_params", "svo_voxel_map_normals_bytes", "svo_voxel_map_normals_dev", "svo_voxel_map_normals",
                  "svo_voxel_map_align_plane_sums_dev", "svo_voxel_map_align_plane_sums_pose7_dev", "svo_voxel_map_align_plane"):
            getattr(L, f).restype = ci
        # the occupancy volume and the locate
        L.svo_voxel_occupancy_bytes.argtypes = [vp, vp]
        L.svo_voxel_map_occupancy_dev.argtypes = [vp, ci, vp, vp, vp, vp]
        L.svo_voxel_map_occupancy.argtypes = [vp, ci, vp, vp, vp, vp]
        L.svo_voxel_map_locate_scores_dev.argtypes = [vp, vp, vp, vp, vp, ci, vp, ci, vp, vp, vp]
        L.svo_voxel_locate_default_params.argtypes = [C.c_float, vp]
        L.svo_voxel_locate_workspace_bytes.argtypes = [vp, vp]
        L.svo_voxel_map_locate.argtypes = [vp, vp, vp, ci, vp, vp, vp, vp, vp, vp]
        for f in ("svo_voxel_occupancy_bytes", "svo_voxel_map_occupancy_dev", "svo_voxel_map_occupancy", "svo_voxel_map_locate_scores_dev",
                  "svo_voxel_locate_default_params", "svo_voxel_locate_workspace_bytes", "svo_voxel_map_locate"):
            getattr(L, f).restype = ci
        # the sight lines
        L.svo_voxel_raycast_default_params.argtypes = [vp]
        L.svo_voxel_occupancy_coarse_bytes.argtypes = [vp, vp]
        L.svo_voxel_occupancy_coarse_dev.argtypes = [vp, vp, vp, vp]
        L.svo_voxel_occupancy_rays_dev.argtypes = [vp, vp, vp, vp, vp, vp, ci, ci, vp, vp]
        L.svo_voxel_occupancy_rays.argtypes = [vp, vp, vp, vp, vp, vp, ci, ci, vp, vp]
        L.svo_voxel_occupancy_raycast_dev.argtypes = [vp, vp, vp, vp, vp, ci, ci, vp, vp, vp, vp, vp, vp]
        L.svo_voxel_occupancy_raycast_pose7_dev.argtypes = [vp, vp, vp, vp, vp, ci, ci, vp, vp, vp, vp, vp, vp]
        L.svo_voxel_map_raycast.argtypes = [vp, ci, vp, ci, ci, vp, vp, vp, vp, vp, vp, vp]
        for f in ("svo_voxel_raycast_default_params", "svo_voxel_occupancy_coarse_bytes", "svo_voxel_occupancy_coarse_dev", "svo_voxel_occupancy_rays_dev",
                  "svo_voxel_occupancy_rays", "svo_voxel_occupancy_raycast_dev", "svo_voxel_occupancy_raycast_pose7_dev", "svo_voxel_map_raycast"):
            getattr(L, f).restype = ci
        # the distance field
        L.svo_voxel_distance_default_params.argtypes = [C.c_float, vp]
        L.svo_voxel_distance_workspace_bytes.argtypes = [vp, ci, vp]
        L.svo_voxel_distance_bytes.argtypes = [vp, vp]
        L.svo_voxel_occupancy_distance_dev.argtypes = [vp, vp, vp, vp, vp, vp, vp]
        L.svo_voxel_distance_query_dev.argtypes = [vp, vp, vp, vp, vp, ci, vp, vp]
        L.svo_voxel_distance_query.argtypes = [vp, vp, vp, vp, vp, ci, vp, vp]
        L.svo_voxel_map_distance.argtypes = [vp, ci, vp, vp, vp, vp, vp]
        for f in ("svo_voxel_distance_default_params", "svo_voxel_distance_workspace_bytes", "svo_voxel_distance_bytes", "svo_voxel_occupancy_distance_dev",
                  "svo_voxel_distance_query_dev", "svo_voxel_distance_query", "svo_voxel_map_distance"):
            getattr(L, f).restype = ci
        # the route through the volume
        L.svo_voxel_route_default_params.argtypes = [C.c_float, vp]
        L.svo_voxel_route_workspace_bytes.argtypes = [vp, vp]
        L.svo_voxel_occupancy_cell_of.argtypes = [C.c_float, vp, vp, vp, vp]
        L.svo_voxel_occupancy_route_dev.argtypes = [vp, vp, vp, vp, vp, vp, ci, vp, ci, vp, vp, vp]
        L.svo_voxel_occupancy_route.argtypes = [vp, vp, vp, vp, vp, vp, ci, vp, ci, vp, vp]
        for f in ("svo_voxel_route_default_params", "svo_voxel_route_workspace_bytes", "svo_voxel_occupancy_cell_of", "svo_voxel_occupancy_route_dev",
                  "svo_voxel_occupancy_route"):
            getattr(L, f).restype = ci
        _LIB = L
    return _LIB


def _p(a, t=None):
    if a is None:
        return None
    return a.ctypes.data_as(C.c_void_p)


def _ref(x):
    """byref(x), or None (a null pointer) for None."""
    return None if x is None else C.byref(x)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _u8(a):
    return np.ascontiguousarray(a, dtype=np.uint8)


def synth_default(width, height):
    p = SynthParams()
    lib().svo_synth_default_params(C.byref(p), width, height)
    return p


def synth_render(params, frame):
    L = lib()
    left = np.empty((params.height, params.width), np.uint8)
    right = np.empty_like(left)
    rc = L.svo_synth_render(C.byref(params), frame, _p(left), _p(right))
    if rc:
        raise SvoError(f"svo_synth_render rc={rc}")
    return left, right


def synth_pose(params, frame):
    rt = np.empty(12, np.float64)
    rc = lib().svo_synth_pose(C.byref(params), frame, _p(rt))
    if rc:
        raise SvoError(f"svo_synth_pose rc={rc}")
    return rt.reshape(3, 4)


class Context:
    """svo_ctx wrapper.  Host-pointer entry points (numpy in/out)."""

    def __init__(self, max_width, max_height, device=0, max_batch=1, max_corners=2048,
                 max_candidates=65536, max_features=2048):
        self.L = lib()
        self.lim = Limits(max_width, max_height, max_batch, max_corners, max_candidates, max_features)
        self.h = C.c_void_p()
        rc = self.L.svo_create(C.byref(self.h), device, C.byref(self.lim))
        if rc:
            raise SvoError(f"svo_create failed rc={rc} (no GPU / HIP error); the HIP path has no fallback")

    def close(self):
        if self.h:
            self.L.svo_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc:
            raise SvoError(f"{what} rc={rc}: {self.L.svo_last_error(self.h).decode()}")

    def sync(self):
        self._chk(self.L.svo_sync(self.h), "svo_sync")

    def cholesky_solve_dev(self, A, b):
        """svo_cholesky_solve_dev on copies (the device-side solve of the LM controller workgroup)."""
        A = np.array(A, np.float64, order="C")
        b = np.array(b, np.float64)
        self._chk(self.L.svo_cholesky_solve_dev(self.h, _p(A), _p(b), b.shape[0]), "svo_cholesky_solve_dev")
        return b

    def profile_select(self, kernel):
        self._chk(self.L.svo_profile_select(self.h, kernel.encode() if kernel else None), "svo_profile_select")

    def profile_read(self):
        ms, n = C.c_double(0), C.c_int(0)
        self._chk(self.L.svo_profile_read(self.h, C.byref(ms), C.byref(n)), "svo_profile_read")
        return ms.value, n.value

    @property
    def stream(self):
        return self.L.svo_stream(self.h)

    # ---- a11
    def measure_peak(self, what):
        """flop/s or bytes/s of this card for "f64_fma" / "f64_muladd" / "f64_mfma" / "hbm_copy" (svo_measure_peak)."""
        v = C.c_double(0.0)
        self._chk(self.L.svo_measure_peak(self.h, what.encode(), C.byref(v)), "svo_measure_peak")
        return v.value

    def reproj_eval(self, pose7, point3, obs2, focal, cx, cy, want_jpose=True, want_jpoint=True):
        pose7, point3, obs2 = _f64(pose7), _f64(point3), _f64(obs2)
        n = pose7.shape[0]
        r = np.empty((n, 2))
        jq = np.empty((n, 14)) if want_jpose else None
        jx = np.empty((n, 6)) if want_jpoint else None
        self._chk(self.L.svo_reproj_eval(self.h, n, _p(pose7), _p(point3), _p(obs2), C.c_double(focal),
                                         C.c_double(cx), C.c_double(cy), _p(r), _p(jq), _p(jx)),
                  "svo_reproj_eval")
        return r, jq, jx

    # ---- a1
    def corner_response(self, img):
        img = _u8(img)
        h, w = img.shape
        eig = np.empty((h, w), np.float32)
        self._chk(self.L.svo_corner_response(self.h, _p(img), w, h, w, _p(eig)), "svo_corner_response")
        return eig

    def corner_detect(self, img, max_corners=300, quality=0.1, min_distance=30.0):
        img = _u8(img)
        h, w = img.shape
        xy = np.empty((max_corners, 2), np.float32)
        n = C.c_int(0)
        self._chk(self.L.svo_corner_detect(self.h, _p(img), w, h, w, max_corners, C.c_double(quality),
                                           C.c_double(min_distance), _p(xy), C.byref(n)),
                  "svo_corner_detect")
        return xy[:n.value].copy()

    def corner_detect_batch_dev(self, imgs, batch, width, height, row_stride, image_stride, max_corners, quality, min_distance, xy, n):
        """svo_corner_detect_batch_dev on torch device tensors: imgs uint8 (batch images, row_stride bytes per row, image_stride bytes
        per image), xy float32 (batch, max_corners, 2), n int32 (batch).  Asynchronous on the context's stream (sync() before reading)."""
        for t, dt in ((imgs, "torch.uint8"), (xy, "torch.float32"), (n, "torch.int32")):
            if not t.is_cuda or not t.is_contiguous() or str(t.dtype) != dt:
                raise SvoError(f"corner_detect_batch_dev: expected a contiguous {dt} device tensor")
        if imgs.numel() < (batch - 1) * image_stride + (height - 1) * row_stride + width or image_stride < row_stride * height:
            raise SvoError("corner_detect_batch_dev: image buffer smaller than the strides say")
        if xy.numel() < batch * max_corners * 2 or n.numel() < batch:
            raise SvoError("corner_detect_batch_dev: output tensors too small")
        self._chk(self.L.svo_corner_detect_batch_dev(self.h, C.c_void_p(imgs.data_ptr()), batch, width, height, row_stride,
                                                     C.c_size_t(image_stride), max_corners, C.c_double(quality), C.c_double(min_distance),
                                                     C.c_void_p(xy.data_ptr()), C.c_void_p(n.data_ptr())), "svo_corner_detect_batch_dev")

    # ---- rectification
    def rectify_remap(self, raw, eye, cam):
        """svo_rectify_remap: raw (H, W) uint8 host image (any row stride) -> rectified (H, W)."""
        raw = np.asarray(raw, np.uint8)
        if raw.strides[1] != 1:
            raw = np.ascontiguousarray(raw)
        h, w = raw.shape
        out = np.empty((h, w), np.uint8)
        self._chk(self.L.svo_rectify_remap(self.h, _p(raw), w, h, raw.strides[0], C.byref(eye), C.byref(cam), _p(out)), "svo_rectify_remap")
        return out

    def rectify_remap_batch_dev(self, raw_ptr, batch, width, height, row_stride, image_stride, eye, cam, out_ptr):
        """svo_rectify_remap_batch_dev: raw device pointers (ints); out: batch tight (H, W) images."""
        self._chk(self.L.svo_rectify_remap_batch_dev(self.h, C.c_void_p(raw_ptr), batch, width, height, row_stride, C.c_size_t(image_stride),
                                                     C.byref(eye), C.byref(cam), C.c_void_p(out_ptr)), "svo_rectify_remap_batch_dev")

    # ---- a7
    def stereo_bm(self, left, right, ndisp=48, block=21):
        left, right = _u8(left), _u8(right)
        h, w = left.shape
        d = np.empty((h, w), np.int16)
        self._chk(self.L.svo_stereo_bm(self.h, _p(left), _p(right), w, h, w, ndisp, block, _p(d)),
                  "svo_stereo_bm")
        return d

    def stereo_disparity_at(self, left, right, xy, ndisp=48, block=21):
        left, right, xy = _u8(left), _u8(right), _f32(xy)
        h, w = left.shape
        n = xy.shape[0]
        d = np.empty(n, np.float32)
        self._chk(self.L.svo_stereo_disparity_at(self.h, _p(left), _p(right), w, h, w, ndisp, block,
                                                 _p(xy), n, _p(d)), "svo_stereo_disparity_at")
        return d

    # ---- dense depth clouds
    def stereo_bm_batch(self, left_ptr, right_ptr, batch, width, height, row_stride, image_stride, disp16_ptr, ndisp=48, block=21):
        """svo_stereo_bm_batch_dev: raw device pointers (ints); disp16_ptr: batch tight (H, W) int16 maps.  Asynchronous."""
        self._chk(self.L.svo_stereo_bm_batch_dev(self.h, left_ptr, right_ptr, batch, width, height, row_stride, image_stride, ndisp, block,
                                                 disp16_ptr), "svo_stereo_bm_batch_dev")

    def disparity_cloud(self, disp16_ptr, left_ptr, batch, width, height, row_stride, image_stride, cam, pose16_ptr, params, points_ptr,
                        counts_ptr):
        """svo_disparity_cloud_batch_dev: raw device pointers (ints; pose16_ptr None = identity); cam: CameraInfo, params: CloudParams;
        points_ptr: batch x params.max_points records of CLOUD_POINT_DTYPE, counts_ptr: batch x 2 int32.  Asynchronous."""
        self._chk(self.L.svo_disparity_cloud_batch_dev(self.h, disp16_ptr, left_ptr, batch, width, height, row_stride, image_stride,
                                                       _ref(cam), pose16_ptr, _ref(params), points_ptr, counts_ptr),
                  "svo_disparity_cloud_batch_dev")

    def stereo_cloud(self, left, right, cam, pose16=None, step=1, min_disparity=0.0, max_points=None, ndisp=48, block=21):
        """svo_stereo_cloud: one host pair -> (points as a CLOUD_POINT_DTYPE array of n_stored records, n_total)."""
        left, right = _u8(left), _u8(right)
        h, w = left.shape
        prm = _cloud_params(w, h, step, min_disparity, max_points)
        pts = np.empty(max(prm.max_points, 1), CLOUD_POINT_DTYPE)
        pose = None if pose16 is None else _f32(pose16).reshape(16)
        nt, ns = C.c_int(0), C.c_int(0)
        self._chk(self.L.svo_stereo_cloud(self.h, _p(left), _p(right), w, h, w, ndisp, block, C.byref(cam), _p(pose), C.byref(prm), _p(pts),
                                          C.byref(nt), C.byref(ns)), "svo_stereo_cloud")
        return pts[:ns.value].copy(), nt.value

    # ---- speckle filter
    def speckle_filter(self, disp16, max_size, max_diff16):
        """svo_disparity_speckle_filter: one host (H, W) int16 map -> (filtered copy, n_removed)."""
        d = np.array(disp16, np.int16, order="C")
        h, w = d.shape
        n = C.c_int(0)
        self._chk(self.L.svo_disparity_speckle_filter(self.h, _p(d), w, h, C.byref(SpeckleParams(int(max_size), int(max_diff16))), C.byref(n)),
                  "svo_disparity_speckle_filter")
        return d, n.value

    def speckle_filter_dev(self, disp16_ptr, batch, width, height, params, workspace_ptr, workspace_bytes, n_removed_ptr=None):
        """svo_disparity_speckle_filter_batch_dev: raw device pointers (ints); disp16_ptr: batch tight (H, W) int16 maps, filtered in
        place; params: SpeckleParams; n_removed_ptr: batch int32 or None.  Asynchronous."""
        self._chk(self.L.svo_disparity_speckle_filter_batch_dev(self.h, disp16_ptr, batch, width, height,
                                                                _ref(params), workspace_ptr, workspace_bytes, n_removed_ptr),
                  "svo_disparity_speckle_filter_batch_dev")

    # ---- left-right check
    def stereo_bm_cost_batch(self, left_ptr, right_ptr, batch, width, height, row_stride, image_stride, disp16_ptr, cost16_ptr,
                             ndisp=48, block=21):
        """svo_stereo_bm_cost_batch_dev: stereo_bm_batch that also writes the winner's SAD per pixel (cost16_ptr: batch tight (H, W)
        uint16 maps, 0xFFFF where the map is FILTERED).  Raw device pointers (ints).  Asynchronous."""
        self._chk(self.L.svo_stereo_bm_cost_batch_dev(self.h, left_ptr, right_ptr, batch, width, height, row_stride, image_stride,
                                                      ndisp, block, disp16_ptr, cost16_ptr), "svo_stereo_bm_cost_batch_dev")

    def lr_check(self, disp16, cost16, max_diff16):
        """svo_disparity_lr_check: one host (H, W) int16 map and its (H, W) uint16 costs -> (checked copy, n_removed)."""
        d = np.array(disp16, np.int16, order="C")
        c = np.ascontiguousarray(cost16, np.uint16)
        h, w = d.shape
        assert c.shape == (h, w)
        n = C.c_int(0)
        self._chk(self.L.svo_disparity_lr_check(self.h, _p(d), _p(c), w, h, C.byref(LrCheckParams(int(max_diff16))), C.byref(n)),
                  "svo_disparity_lr_check")
        return d, n.value

    def lr_check_dev(self, disp16_ptr, cost16_ptr, batch, width, height, params, n_removed_ptr=None):
        """svo_disparity_lr_check_batch_dev: raw device pointers (ints); disp16_ptr: batch tight (H, W) int16 maps, checked in place;
        cost16_ptr: their uint16 costs; params: LrCheckParams; n_removed_ptr: batch int32 or None.  Asynchronous."""
        self._chk(self.L.svo_disparity_lr_check_batch_dev(self.h, disp16_ptr, cost16_ptr, batch, width, height,
                                                          _ref(params), n_removed_ptr),
                  "svo_disparity_lr_check_batch_dev")

    # ---- semi-global matching
    def sgm_workspace_bytes(self, width, height, ndisp=48, block=21, batch=1):
        """svo_sgm_workspace_bytes (see the module function of the same name)."""
        return sgm_workspace_bytes(width, height, ndisp, block, batch)

    def stereo_sgm(self, left, right, ndisp=48, block=21, p1=None, p2=None, cost=False):
        """svo_stereo_sgm: one host pair -> the (H, W) int16 map, or (map, (H, W) uint16 cost) with cost=True.  p1 / p2 None: the
        defaults 2 block^2 / 8 block^2."""
        left, right = _u8(left), _u8(right)
        h, w = left.shape
        d = np.empty((h, w), np.int16)
        c = np.empty((h, w), np.uint16) if cost else None
        prm = _sgm_params(p1, p2, block)
        self._chk(self.L.svo_stereo_sgm(self.h, _p(left), _p(right), w, h, w, ndisp, block, C.byref(prm), _p(d), _p(c)), "svo_stereo_sgm")
        return (d, c) if cost else d

    def stereo_sgm_batch(self, left_ptr, right_ptr, batch, width, height, row_stride, image_stride, params, workspace_ptr, workspace_bytes,
                         disp16_ptr, cost16_ptr=None, ndisp=48, block=21):
        """svo_stereo_sgm_batch_dev: raw device pointers (ints); params: SgmParams; workspace: sgm_workspace_bytes(...) bytes;
        disp16_ptr: batch tight (H, W) int16 maps; cost16_ptr: batch tight (H, W) uint16 maps or None.  Asynchronous."""
        self._chk(self.L.svo_stereo_sgm_batch_dev(self.h, left_ptr, right_ptr, batch, width, height, row_stride, image_stride, ndisp, block,
                                                  _ref(params), workspace_ptr, workspace_bytes, disp16_ptr, cost16_ptr),
                  "svo_stereo_sgm_batch_dev")

    # ---- ground plan surface
    def grid_surface(self, cls_ptr, top_ptr, params, cls_out_ptr=None, step_ptr=None, relief_ptr=None, support_ptr=None, counts_ptr=None,
                     **overrides):
        """svo_grid_surface_dev: per cell of the na x nb grid behind cls_ptr (uint8) and top_ptr (float32, the grid's top) the largest
        height step to an edge neighbour, the relief and the support under the footprint, and the refined class grid (STEP 3, ROUGH 4,
        UNSUPPORTED 5).  params (a GridSurfaceParams) and / or its fields as keywords.  All pointers are the caller's device memory:
        cls_out_ptr na * nb uint8 (required, not cls_ptr), step_ptr and relief_ptr float32, support_ptr uint16 or None each,
        counts_ptr 6 uint64 GRID_SURFACE_COUNTS or None.  Asynchronous on the context's stream; returns {"cls_out", "step", "relief",
        "support", "counts", "na", "nb"}: the pointers the outputs are behind once the stream reaches this point."""
        prm = _params(GridSurfaceParams, params, **overrides)
        out = GridSurfaceOut(cls_out_ptr, step_ptr, relief_ptr, support_ptr)
        self._chk(self.L.svo_grid_surface_dev(self.h, cls_ptr, top_ptr, C.byref(prm), C.byref(out), counts_ptr), "svo_grid_surface_dev")
        return {"cls_out": cls_out_ptr, "step": step_ptr, "relief": relief_ptr, "support": support_ptr, "counts": counts_ptr,
                "na": prm.na, "nb": prm.nb}

    def grid_surface_host(self, cls, top, params, **overrides):
        """svo_grid_surface: synchronous.  cls: an (na, nb) uint8 array, top: float32 of the same shape.  Returns (cls_out (na, nb)
        uint8, step and relief float32 (-1 where the cell is not ground), support uint16, {GRID_SURFACE_COUNTS})."""
        cls = np.ascontiguousarray(cls, np.uint8)
        top = np.ascontiguousarray(top, np.float32)
        if cls.ndim != 2 or top.shape != cls.shape:
            raise ValueError("grid_surface_host: cls and top must be (na, nb) arrays of one shape")
        prm = _params(GridSurfaceParams, params, **overrides)
        if (prm.na, prm.nb) != cls.shape:
            raise ValueError(f"grid_surface_host: cls is {cls.shape}, the parameters say {(prm.na, prm.nb)}")
        arrays = [np.empty(cls.shape, t) for t in (np.uint8, np.float32, np.float32, np.uint16)]
        out = GridSurfaceOut(*(a.ctypes.data for a in arrays))
        c = np.zeros(6, np.uint64)
        self._chk(self.L.svo_grid_surface(self.h, _p(cls), _p(top), C.byref(prm), C.byref(out), _p(c)), "svo_grid_surface")
        return (*arrays, dict(zip(GRID_SURFACE_COUNTS, (int(v) for v in c))))

    # ---- ground plan clearance
    def grid_clearance(self, cls_ptr, params=None, workspace_ptr=None, dist2_ptr=None, nearest_ptr=None, clearance_ptr=None, blocked_ptr=None,
                       counts_ptr=None, **overrides):
        """svo_grid_clearance_dev: per cell of the na x nb uint8 class grid behind cls_ptr the squared distance in cells to the nearest
        source cell, that cell's index, the distance in map units and the inflation.  params (a GridClearanceParams) and / or its
        fields as keywords.  All pointers are the caller's device memory: workspace_ptr grid_clearance_workspace_bytes(na, nb) bytes,
        dist2_ptr na * nb uint32 (required), nearest_ptr uint32, clearance_ptr float32, blocked_ptr uint8 or None each, counts_ptr 4
        uint64 GRID_CLEARANCE_COUNTS or None.  Asynchronous on the context's stream; returns {"dist2", "nearest", "clearance",
        "blocked", "counts", "workspace", "na", "nb"}: the pointers the outputs are behind once the stream reaches this point."""
        prm = _clearance_params(params, overrides)
        out = GridClearanceOut(dist2_ptr, nearest_ptr, clearance_ptr, blocked_ptr)
        self._chk(self.L.svo_grid_clearance_dev(self.h, cls_ptr, C.byref(prm), workspace_ptr, C.byref(out), counts_ptr), "svo_grid_clearance_dev")
        return {"dist2": dist2_ptr, "nearest": nearest_ptr, "clearance": clearance_ptr, "blocked": blocked_ptr, "counts": counts_ptr,
                "workspace": workspace_ptr, "na": prm.na, "nb": prm.nb}

    def grid_clearance_host(self, cls, params=None, **overrides):
        """svo_grid_clearance: synchronous.  cls: an (na, nb) uint8 array (na and nb are taken from it unless given).  Returns (dist2
        and nearest (na, nb) uint32 with GRID_CLEARANCE_NONE where no source is within max_dist, clearance float32 (+inf there),
        blocked uint8 (2 a source, 1 inside the inflation, 0 free), {GRID_CLEARANCE_COUNTS})."""
        cls = np.ascontiguousarray(cls, np.uint8)
        if cls.ndim != 2:
            raise ValueError("grid_clearance_host: cls must be an (na, nb) array")
        if params is None:
            overrides = {"na": cls.shape[0], "nb": cls.shape[1], **overrides}
        prm = _clearance_params(params, overrides)
        if (prm.na, prm.nb) != cls.shape:
            raise ValueError(f"grid_clearance_host: cls is {cls.shape}, the parameters say {(prm.na, prm.nb)}")
        arrays = [np.empty(cls.shape, t) for t in (np.uint32, np.uint32, np.float32, np.uint8)]
        out = GridClearanceOut(*(a.ctypes.data for a in arrays))
        c = np.zeros(4, np.uint64)
        self._chk(self.L.svo_grid_clearance(self.h, _p(cls), C.byref(prm), C.byref(out), _p(c)), "svo_grid_clearance")
        return (*arrays, dict(zip(GRID_CLEARANCE_COUNTS, (int(v) for v in c))))

    # ---- ground plan route
    def grid_route(self, blocked_ptr, params, goals_ptr, n_goals, workspace_ptr=None, cost_ptr=None, dist2_ptr=None, next_ptr=None,
                   starts_ptr=None, n_starts=0, path_ptr=None, path_len_ptr=None, path_status_ptr=None, counts_ptr=None, **overrides):
        """svo_grid_route_dev: the cost-to-go field to the goal cells over the na x nb uint8 grid behind blocked_ptr (passable iff 0),
        the first move per cell and the paths from the start cells.  params (a GridRouteParams) and / or its fields as keywords.  All
        pointers are the caller's device memory: workspace_ptr grid_route_workspace_bytes(na, nb) bytes, cost_ptr na * nb uint32
        (required), dist2_ptr na * nb uint32, next_ptr na * nb uint8, goals_ptr n_goals and starts_ptr n_starts uint32 cell indices,
        path_ptr n_starts x max_path uint32, path_len_ptr uint32 and path_status_ptr uint8 per start (the three together or None),
        counts_ptr 8 uint64 (GRID_ROUTE_COUNTS and two zeros) or None.  Asynchronous on the context's stream; returns the pointers
        the outputs are behind once the stream reaches this point, with "workspace", "na", "nb"."""
        prm = _route_params(params, overrides)
        out = GridRouteOut(cost_ptr, next_ptr, path_ptr, path_len_ptr, path_status_ptr)
        self._chk(self.L.svo_grid_route_dev(self.h, blocked_ptr, dist2_ptr, C.byref(prm), goals_ptr, int(n_goals), starts_ptr, int(n_starts),
                                            workspace_ptr, C.byref(out), counts_ptr), "svo_grid_route_dev")
        return {"cost": cost_ptr, "next": next_ptr, "path": path_ptr, "path_len": path_len_ptr, "path_status": path_status_ptr,
                "counts": counts_ptr, "workspace": workspace_ptr, "na": prm.na, "nb": prm.nb}

    def grid_route_host(self, blocked, goals, dist2=None, starts=None, params=None, **overrides):
        """svo_grid_route: synchronous.  blocked: an (na, nb) uint8 array (na and nb are taken from it unless given); goals, starts:
        cell indices; dist2: (na, nb) uint32 or None.  Returns {"cost" (na, nb) uint32 with GRID_ROUTE_NONE, "next" (na, nb) uint8,
        "counts" {GRID_ROUTE_COUNTS}} and, with starts, "path" (n_starts, max_path) uint32 (GRID_ROUTE_NONE where nothing was
        written), "path_len" uint32 and "path_status" uint8 per start."""
        blocked = np.ascontiguousarray(blocked, np.uint8)
        if blocked.ndim != 2:
            raise ValueError("grid_route_host: blocked must be an (na, nb) array")
        if params is None:
            overrides = {"na": blocked.shape[0], "nb": blocked.shape[1], **overrides}
        prm = _route_params(params, overrides)
        if (prm.na, prm.nb) != blocked.shape:
            raise ValueError(f"grid_route_host: blocked is {blocked.shape}, the parameters say {(prm.na, prm.nb)}")
        if dist2 is not None:
            dist2 = np.ascontiguousarray(dist2, np.uint32)
            if dist2.shape != blocked.shape:
                raise ValueError("grid_route_host: dist2 must have the shape of blocked")
        goals = np.ascontiguousarray(goals, np.uint32).ravel()
        starts = None if starts is None else np.ascontiguousarray(starts, np.uint32).ravel()
        ns = 0 if starts is None else len(starts)
        res = {"cost": np.empty(blocked.shape, np.uint32), "next": np.full(blocked.shape, 255, np.uint8)}
        if ns:
            if not 1 <= prm.max_path <= 1 << 20:
                raise SvoError("svo_grid_route: grid_route: max_path outside 1..2^20")
            res.update(path=np.full((ns, prm.max_path), GRID_ROUTE_NONE, np.uint32), path_len=np.zeros(ns, np.uint32), path_status=np.zeros(ns, np.uint8))
        out = GridRouteOut(*(res[k].ctypes.data if k in res else None for k in ("cost", "next", "path", "path_len", "path_status")))
        c = np.zeros(8, np.uint64)
        self._chk(self.L.svo_grid_route(self.h, _p(blocked), _p(dist2), C.byref(prm), _p(goals), len(goals), _p(starts) if ns else None, ns,
                                        C.byref(out), _p(c)), "svo_grid_route")
        res["counts"] = dict(zip(GRID_ROUTE_COUNTS, (int(v) for v in c)))
        return res

    # ---- ground plan frontiers
    def grid_frontiers(self, cls_ptr, params=None, blocked_ptr=None, cost_ptr=None, workspace_ptr=None, frontiers_ptr=None, goal_cells_ptr=None,
                       label_ptr=None, counts_ptr=None, **overrides):
        """svo_grid_frontiers_dev: the frontiers of the na x nb uint8 class grid behind cls_ptr: FREE cells (off the cells blocked_ptr
        marks) with an UNKNOWN edge neighbour, in 8-connected pieces.  params (a GridFrontierParams) and / or its fields as keywords.
        All pointers are the caller's device memory: blocked_ptr na * nb uint8 or None, cost_ptr na * nb uint32 (a route's cost) or
        None, workspace_ptr grid_frontier_workspace_bytes(na, nb, max_frontiers) bytes, frontiers_ptr max_frontiers records of
        GRID_FRONTIER_DTYPE, goal_cells_ptr max_frontiers uint32 (fits grid_route's goals_ptr with n_goals = max_frontiers), label_ptr
        na * nb uint32 (at least one of the three), counts_ptr 8 uint64 (GRID_FRONTIER_COUNTS and a zero) or None.  Asynchronous on
        the context's stream; returns the pointers the outputs are behind once the stream reaches this point, with "workspace", "na",
        "nb", "max_frontiers"."""
        prm = _frontier_params(params, overrides)
        out = GridFrontierOut(frontiers_ptr, goal_cells_ptr, label_ptr)
        self._chk(self.L.svo_grid_frontiers_dev(self.h, cls_ptr, blocked_ptr, cost_ptr, C.byref(prm), workspace_ptr, C.byref(out), counts_ptr),
                  "svo_grid_frontiers_dev")
        return {"frontiers": frontiers_ptr, "goal_cells": goal_cells_ptr, "label": label_ptr, "counts": counts_ptr, "workspace": workspace_ptr,
                "na": prm.na, "nb": prm.nb, "max_frontiers": prm.max_frontiers}

    def grid_frontiers_host(self, cls, blocked=None, cost=None, params=None, **overrides):
        """svo_grid_frontiers: synchronous.  cls: an (na, nb) uint8 array (na and nb are taken from it unless given); blocked: (na, nb)
        uint8 or None; cost: (na, nb) uint32 or None.  Returns {"frontiers": the n_written records as a structured array of
        GRID_FRONTIER_DTYPE, "goal_cells" (max_frontiers,) uint32 padded with GRID_FRONTIER_NONE, "label" (na, nb) uint32, "counts"
        {GRID_FRONTIER_COUNTS}}."""
        cls = np.ascontiguousarray(cls, np.uint8)
        if cls.ndim != 2:
            raise ValueError("grid_frontiers_host: cls must be an (na, nb) array")
        if params is None:
            overrides = {"na": cls.shape[0], "nb": cls.shape[1], **overrides}
        prm = _frontier_params(params, overrides)
        if (prm.na, prm.nb) != cls.shape:
            raise ValueError(f"grid_frontiers_host: cls is {cls.shape}, the parameters say {(prm.na, prm.nb)}")
        if blocked is not None:
            blocked = np.ascontiguousarray(blocked, np.uint8)
            if blocked.shape != cls.shape:
                raise ValueError("grid_frontiers_host: blocked must have the shape of cls")
        if cost is not None:
            cost = np.ascontiguousarray(cost, np.uint32)
            if cost.shape != cls.shape:
                raise ValueError("grid_frontiers_host: cost must have the shape of cls")
        if not 1 <= prm.max_frontiers <= 65536:
            raise SvoError("svo_grid_frontiers: grid_frontier: max_frontiers outside 1..65536")
        rec = np.zeros(prm.max_frontiers, GRID_FRONTIER_DTYPE)
        goal = np.empty(prm.max_frontiers, np.uint32)
        label = np.empty(cls.shape, np.uint32)
        out = GridFrontierOut(rec.ctypes.data, goal.ctypes.data, label.ctypes.data)
        c = np.zeros(8, np.uint64)
        self._chk(self.L.svo_grid_frontiers(self.h, _p(cls), _p(blocked), _p(cost), C.byref(prm), C.byref(out), _p(c)), "svo_grid_frontiers")
        counts = dict(zip(GRID_FRONTIER_COUNTS, (int(v) for v in c)))
        return {"frontiers": rec[:counts["n_written"]].copy(), "goal_cells": goal, "label": label, "counts": counts}

    def grid_frontier_set_mode(self, combine=None):
        """svo_grid_frontier_set_mode (measurement aid): whether runs of equal rank along a wavefront are combined before the
        per-frontier atomics; no bit of a result depends on it.  None: the default."""
        self._chk(self.L.svo_grid_frontier_set_mode(self.h, int(GRID_FRONTIER_COMBINE_DEFAULT if combine is None else bool(combine))),
                  "svo_grid_frontier_set_mode")

    # ---- ground plan view
    def grid_view(self, cls_ptr, views_ptr, n_views, params=None, cost_ptr=None, workspace_ptr=None, records_ptr=None, order_ptr=None,
                  best_ptr=None, seen_ptr=None, counts_ptr=None, **overrides):
        """svo_grid_view_dev: what each of the n_views uint32 cells behind views_ptr (the frontiers' goal_cells fit as they are) would
        see of the na x nb uint8 class grid behind cls_ptr, scored against the uint32 cost field behind cost_ptr (a route's cost) where
        given, ranked, and the best one named.  All device pointers: cost_ptr na * nb uint32 or None, workspace_ptr
        grid_view_workspace_bytes(na, nb, n_views) bytes, records_ptr n_views records of GRID_VIEW_DTYPE, order_ptr n_views uint32,
        best_ptr 4 uint32 (GRID_VIEW_BEST; its first word fits grid_route's goals_ptr with n_goals = 1), seen_ptr na * nb uint32 (at
        least one of the four), counts_ptr 8 uint64 (GRID_VIEW_COUNTS and a zero) or None.  Asynchronous on the context's stream.
        Returns the pointers and "na", "nb", "n_views"."""
        prm = _view_params(params, overrides)
        out = GridViewOut(records_ptr, order_ptr, best_ptr, seen_ptr)
        self._chk(self.L.svo_grid_view_dev(self.h, cls_ptr, views_ptr, int(n_views), cost_ptr, C.byref(prm), workspace_ptr, C.byref(out), counts_ptr),
                  "svo_grid_view_dev")
        return {"records": records_ptr, "order": order_ptr, "best": best_ptr, "seen": seen_ptr, "counts": counts_ptr, "workspace": workspace_ptr,
                "na": prm.na, "nb": prm.nb, "n_views": int(n_views)}

    def grid_view_host(self, cls, views, cost=None, params=None, **overrides):
        """svo_grid_view: synchronous.  cls: an (na, nb) uint8 array (na and nb are taken from it unless given); views: 1..4096 uint32
        cell indices; cost: (na, nb) uint32 or None.  Returns {"records": a structured array of GRID_VIEW_DTYPE, one per view, "order"
        (n_views,) uint32, "best" {GRID_VIEW_BEST}, "seen" (na, nb) uint32, "counts" {GRID_VIEW_COUNTS}}."""
        cls = np.ascontiguousarray(cls, np.uint8)
        if cls.ndim != 2:
            raise ValueError("grid_view_host: cls must be an (na, nb) array")
        if params is None:
            overrides = {"na": cls.shape[0], "nb": cls.shape[1], **overrides}
        prm = _view_params(params, overrides)
        if (prm.na, prm.nb) != cls.shape:
            raise ValueError(f"grid_view_host: cls is {cls.shape}, the parameters say {(prm.na, prm.nb)}")
        views = np.ascontiguousarray(views, np.uint32).ravel()
        if cost is not None:
            cost = np.ascontiguousarray(cost, np.uint32)
            if cost.shape != cls.shape:
                raise ValueError("grid_view_host: cost must have the shape of cls")
        if not 1 <= len(views) <= GRID_VIEW_MAX_VIEWS:
            raise SvoError("svo_grid_view: grid_view: n_views outside 1..4096")
        rec = np.zeros(len(views), GRID_VIEW_DTYPE)
        order = np.empty(len(views), np.uint32)
        best = np.empty(4, np.uint32)
        seen = np.empty(cls.shape, np.uint32)
        out = GridViewOut(rec.ctypes.data, order.ctypes.data, best.ctypes.data, seen.ctypes.data)
        c = np.zeros(8, np.uint64)
        self._chk(self.L.svo_grid_view(self.h, _p(cls), _p(views), len(views), _p(cost), C.byref(prm), C.byref(out), _p(c)), "svo_grid_view")
        return {"records": rec, "order": order, "best": dict(zip(GRID_VIEW_BEST, (int(v) for v in best))), "seen": seen,
                "counts": dict(zip(GRID_VIEW_COUNTS, (int(v) for v in c)))}

    def grid_view_set_mode(self, staged=None):
        """svo_grid_view_set_mode (measurement aid): whether a view's lines are walked over bit planes of its window staged in LDS or
        over cls in global memory; no bit of a result depends on it.  None: the default."""
        self._chk(self.L.svo_grid_view_set_mode(self.h, int(GRID_VIEW_STAGED_DEFAULT if staged is None else bool(staged))), "svo_grid_view_set_mode")

    # ---- ground plan waypoints
    def grid_waypoints(self, blocked_ptr, path_ptr, path_len_ptr, n_paths, params, dist2_ptr=None, path_status_ptr=None, way_ptr=None,
                       way_index_ptr=None, way_len_ptr=None, way_status_ptr=None, length_ptr=None, counts_ptr=None):
        """svo_grid_waypoints_dev: per path of a route (path_ptr n_paths * path_stride uint32, path_len_ptr n_paths uint32,
        path_status_ptr n_paths uint8 or None: grid_route's outputs as they are) the few cells between which a vehicle may drive in
        straight lines over the na x nb uint8 grid behind blocked_ptr (passable iff 0; dist2_ptr na * nb uint32 or None).  params: a
        GridWaypointParams.  All device pointers: way_ptr and way_index_ptr n_paths * max_way uint32, way_len_ptr n_paths uint32,
        way_status_ptr n_paths uint8, length_ptr n_paths float64 (at least one; way and way_len together), counts_ptr 8 uint64
        (GRID_WAY_COUNTS and a zero) or None.  Asynchronous on the context's stream.  Returns the pointers and "n_paths", "max_way"."""
        out = GridWaypointOut(way_ptr, way_index_ptr, way_len_ptr, way_status_ptr, length_ptr)
        self._chk(self.L.svo_grid_waypoints_dev(self.h, blocked_ptr, dist2_ptr, path_ptr, path_len_ptr, path_status_ptr, int(n_paths), C.byref(params),
                                                C.byref(out), counts_ptr), "svo_grid_waypoints_dev")
        return {"way": way_ptr, "way_index": way_index_ptr, "way_len": way_len_ptr, "way_status": way_status_ptr, "length": length_ptr,
                "counts": counts_ptr, "n_paths": int(n_paths), "max_way": params.max_way}

    def grid_waypoints_host(self, blocked, path, path_len, params, dist2=None, path_status=None):
        """svo_grid_waypoints: synchronous.  blocked: an (na, nb) uint8 array; path: (n_paths, path_stride) uint32; path_len: (n_paths,)
        uint32; dist2: (na, nb) uint32 or None; path_status: (n_paths,) uint8 or None.  Returns {"way" and "way_index" (n_paths,
        max_way) uint32 with GRID_WAY_NONE where nothing was written, "way_len" (n_paths,) uint32, "way_status" (n_paths,) uint8,
        "length" (n_paths,) float64, "counts" {GRID_WAY_COUNTS}}."""
        blocked = np.ascontiguousarray(blocked, np.uint8)
        if blocked.shape != (params.na, params.nb):
            raise ValueError(f"grid_waypoints_host: blocked is {blocked.shape}, the parameters say {(params.na, params.nb)}")
        path = np.ascontiguousarray(path, np.uint32)
        path_len = np.ascontiguousarray(path_len, np.uint32).ravel()
        n_paths = len(path_len)
        if path.ndim != 2 or path.shape != (n_paths, params.path_stride):
            raise ValueError(f"grid_waypoints_host: path is {path.shape}, path_len and the parameters say {(n_paths, params.path_stride)}")
        if dist2 is not None:
            dist2 = np.ascontiguousarray(dist2, np.uint32)
            if dist2.shape != blocked.shape:
                raise ValueError("grid_waypoints_host: dist2 must have the shape of blocked")
        if path_status is not None:
            path_status = np.ascontiguousarray(path_status, np.uint8).ravel()
            if len(path_status) != n_paths:
                raise ValueError("grid_waypoints_host: path_status must have one entry per path")
        if not 1 <= n_paths <= GRID_WAY_MAX_PATHS:
            raise SvoError("svo_grid_waypoints: grid_waypoints: n_paths outside 1..4096")
        if not 1 <= params.max_way <= 1 << 20:
            raise SvoError("svo_grid_waypoints: grid_waypoints: max_way outside 1..2^20")
        way = np.full((n_paths, params.max_way), GRID_WAY_NONE, np.uint32)
        index = np.full((n_paths, params.max_way), GRID_WAY_NONE, np.uint32)
        wlen, status, length = np.empty(n_paths, np.uint32), np.empty(n_paths, np.uint8), np.empty(n_paths, np.float64)
        out = GridWaypointOut(way.ctypes.data, index.ctypes.data, wlen.ctypes.data, status.ctypes.data, length.ctypes.data)
        c = np.zeros(8, np.uint64)
        self._chk(self.L.svo_grid_waypoints(self.h, _p(blocked), _p(dist2), _p(path), _p(path_len), _p(path_status), n_paths, C.byref(params),
                                            C.byref(out), _p(c)), "svo_grid_waypoints")
        return {"way": way, "way_index": index, "way_len": wlen, "way_status": status, "length": length,
                "counts": dict(zip(GRID_WAY_COUNTS, (int(v) for v in c)))}

    # ---- a8
    def triangulate(self, xy, disp, pose16, focal, cx, cy, baseline):
        xy, disp, pose16 = _f32(xy), _f32(disp), _f32(pose16)
        n = xy.shape[0]
        kxy = np.empty((n, 2), np.float32)
        xyz = np.empty((n, 3), np.float32)
        kidx = np.empty(n, np.int32)
        m = C.c_int(0)
        self._chk(self.L.svo_triangulate(self.h, _p(xy), _p(disp), n, _p(pose16), C.c_float(focal),
                                         C.c_float(cx), C.c_float(cy), C.c_float(baseline), _p(kxy),
                                         _p(xyz), _p(kidx), C.byref(m)), "svo_triangulate")
        return kxy[:m.value].copy(), xyz[:m.value].copy(), kidx[:m.value].copy()

    # ---- a3
    def build_pyramid(self, img):
        img = _u8(img)
        h, w = img.shape
        sizes = []
        lw, lh = w, h
        for _ in range(4):
            sizes.append((lh, lw))
            lw, lh = (lw + 1) // 2, (lh + 1) // 2
        total = sum(a * b for a, b in sizes)
        buf = np.empty(total, np.uint8)
        self._chk(self.L.svo_build_pyramid(self.h, _p(img), w, h, w, _p(buf), C.c_size_t(total)),
                  "svo_build_pyramid")
        out, off = [], 0
        for (a, b) in sizes:
            out.append(buf[off:off + a * b].reshape(a, b).copy())
            off += a * b
        return out

    def lk_track(self, prev, nxt, xy):
        prev, nxt, xy = _u8(prev), _u8(nxt), _f32(xy)
        h, w = prev.shape
        n = xy.shape[0]
        out = np.empty((n, 2), np.float32)
        st = np.empty(n, np.uint8)
        self._chk(self.L.svo_lk_track(self.h, _p(prev), _p(nxt), w, h, w, _p(xy), n, _p(out), _p(st)),
                  "svo_lk_track")
        return out, st

    def track_features(self, prev, nxt, xy, initial_xy):
        prev, nxt, xy, initial_xy = _u8(prev), _u8(nxt), _f32(xy), _f32(initial_xy)
        h, w = prev.shape
        n = xy.shape[0]
        kxy = np.empty((n, 2), np.float32)
        kidx = np.empty(n, np.int32)
        m = C.c_int(0)
        av = C.c_float(0)
        self._chk(self.L.svo_track_features(self.h, _p(prev), _p(nxt), w, h, w, _p(xy), _p(initial_xy), n,
                                            _p(kxy), _p(kidx), C.byref(m), C.byref(av)),
                  "svo_track_features")
        return kxy[:m.value].copy(), kidx[:m.value].copy(), av.value

    # ---- a6
    def dedup(self, det, trk, min_distance):
        det, trk = _f32(det), _f32(trk)
        out = np.empty_like(det)
        m = C.c_int(0)
        self._chk(self.L.svo_dedup(self.h, _p(det), det.shape[0], _p(trk), trk.shape[0],
                                   C.c_float(min_distance), _p(out), C.byref(m)), "svo_dedup")
        return out[:m.value].copy()

    # ---- a5
    def pnp_ransac(self, xyz, xy, focal, cx, cy, rvec, tvec, iterations=100, reproj_err=8.0, confidence=0.99):
        xyz, xy = _f32(xyz), _f32(xy)
        n = xyz.shape[0]
        rv, tv = _f64(rvec).copy(), _f64(tvec).copy()
        inl = np.empty(max(n, 1), np.int32)
        m = C.c_int(0)
        self._chk(self.L.svo_pnp_ransac(self.h, _p(xyz), _p(xy), n, C.c_float(focal), C.c_float(cx),
                                        C.c_float(cy), _p(rv), _p(tv), iterations, C.c_float(reproj_err),
                                        C.c_double(confidence), _p(inl), C.byref(m)), "svo_pnp_ransac")
        return rv, tv, inl[:m.value].copy()


class VoxelMap:
    """svo_voxel_map: a device-resident sparse voxel grid that fuses clouds into one world-frame map (include/svo.h, "voxel map").
    Close it before its context."""

    def __init__(self, ctx, params=None, voxel_size=None, capacity_log2=None, max_depth=None):
        self.ctx, self.L = ctx, ctx.L
        prm = _params(voxel_map_default_params, params, voxel_size=voxel_size, capacity_log2=capacity_log2, max_depth=max_depth)
        self.params = prm
        self.h = C.c_void_p()
        ctx._chk(self.L.svo_voxel_map_create(ctx.h, C.byref(prm), C.byref(self.h)), "svo_voxel_map_create")
        self.capacity = 1 << prm.capacity_log2

    def close(self):
        if self.h:
            if self.ctx.h:  # a map that outlived its context cannot be destroyed any more (its table went with the device memory)
                self.L.svo_voxel_map_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def clear(self):
        self.ctx._chk(self.L.svo_voxel_map_clear(self.h), "svo_voxel_map_clear")

    def _by_pose(self, who, name, matrix, pose7, entry, head, tail=(), to_matrix=None):
        """Exactly one of the 3 x 4 matrix (the argument called `name`) and pose7: svo_voxel_map_<entry>_dev(map, *head, matrix, *tail)
        or its _pose7_dev form; for an entry that has no pose7 form, to_matrix makes the matrix and svo_voxel_map_<entry> is called."""
        if (matrix is None) == (pose7 is None):
            raise ValueError(f"VoxelMap.{who}: give exactly one of {name} and pose7")
        if to_matrix is not None:
            fn, a = "svo_voxel_map_" + entry, _f64(to_matrix(pose7) if matrix is None else matrix).reshape(12)
        elif pose7 is None:
            fn, a = f"svo_voxel_map_{entry}_dev", _f64(matrix).reshape(12)
        else:
            fn, a = f"svo_voxel_map_{entry}_pose7_dev", _f64(pose7).reshape(7)
        self.ctx._chk(getattr(self.L, fn)(self.h, *head, _p(a), *tail), fn)

    def insert(self, dev_ptr, n, m12=None, pose7=None):
        """n CLOUD_POINT_DTYPE records at the device pointer (an int) under m12 (3 x 4 camera->world) or pose7, exactly one of them.
        Asynchronous on the context's stream."""
        self._by_pose("insert", "m12", m12, pose7, "insert", (dev_ptr, int(n)))

    def remove(self, dev_ptr, n, m12=None, pose7=None, counts_ptr=None):
        """svo_voxel_map_remove_dev / _pose7_dev: the n records at the device pointer taken back out under m12 or pose7 (exactly one):
        the exact inverse of the insert that had the same records and the same matrix bits.  counts_ptr: 4 uint64 on the device
        {n_removed, n_rejected, n_missing, n_short}, or None.  Asynchronous on the context's stream."""
        self._by_pose("remove", "m12", m12, pose7, "remove", (dev_ptr, int(n)), (counts_ptr,))

    def remove_host_counts(self, dev_ptr, n, m12=None, pose7=None):
        """remove() with counts of its own, synchronous: returns {"n_removed", "n_rejected", "n_missing", "n_short"}."""
        c = np.zeros(4, np.uint64)
        self._by_pose("remove_host_counts", "m12", m12, pose7, "remove_sync", (dev_ptr, int(n)), (_p(c),), pose7_to_cam_to_world)
        return dict(zip(REMOVE_COUNTS, (int(v) for v in c)))

    def move(self, dev_ptr, n, from_m12=None, to_m12=None, from_pose7=None, to_pose7=None, counts_ptr=None):
        """svo_voxel_map_move_dev / _pose7_dev: the removal under from_..., then the insert under to_... (both as m12 or both as
        pose7).  Matrices equal in every bit launch nothing.  counts_ptr: the removal's counts, or None.  Asynchronous."""
        by_m, by_q = from_m12 is not None and to_m12 is not None, from_pose7 is not None and to_pose7 is not None
        if by_m == by_q or (by_m and (from_pose7 is not None or to_pose7 is not None)) or (by_q and (from_m12 is not None or to_m12 is not None)):
            raise ValueError("VoxelMap.move: give from_m12 and to_m12, or from_pose7 and to_pose7")
        if by_m:
            a, b = _f64(from_m12).reshape(12), _f64(to_m12).reshape(12)
            self.ctx._chk(self.L.svo_voxel_map_move_dev(self.h, dev_ptr, int(n), _p(a), _p(b), counts_ptr), "svo_voxel_map_move_dev")
        else:
            a, b = _f64(from_pose7).reshape(7), _f64(to_pose7).reshape(7)
            self.ctx._chk(self.L.svo_voxel_map_move_pose7_dev(self.h, dev_ptr, int(n), _p(a), _p(b), counts_ptr), "svo_voxel_map_move_pose7_dev")

    def align_sums(self, points_ptr, n, c2w12=None, pose7=None, params=None, sums_ptr=None, **overrides):
        """svo_voxel_map_align_sums_dev / _pose7_dev: the n records at the device pointer matched against the map under c2w12 (3 x 4
        camera->world) or pose7, exactly one of them; the normal equations of the pose increment and the four counts go to the 32
        int64 at the device pointer sums_ptr (include/svo.h, "Voxel map align").  params: a VoxelAlignParams (None: the defaults for
        this map's voxel size) and / or its fields as keywords.  Nothing in the map changes.  Asynchronous on the context's stream."""
        prm = _params(lambda: voxel_align_default_params(self.params.voxel_size), params, **overrides)
        self._by_pose("align_sums", "c2w12", c2w12, pose7, "align_sums", (points_ptr, int(n)), (C.byref(prm), sums_ptr))

    def align(self, points_ptr, n, pose7, params=None, **overrides):
        """svo_voxel_map_align: the pose7 of the cloud at the device pointer refined against the map by the host-driven loop;
        synchronous.  Align a keyframe's cloud BEFORE inserting it, then insert it under the result.  Returns (pose7_out as 7
        float64, {"status" (one of VOXEL_ALIGN_STATUS), "iterations", "first_matched", "last_matched", "first_cost", "last_cost",
        "xi" (6 float64)})."""
        prm = _params(lambda: voxel_align_default_params(self.params.voxel_size), params, **overrides)
        q = _f64(pose7).reshape(7)
        out, res = np.empty(7, np.float64), VoxelAlignResult()
        self.ctx._chk(self.L.svo_voxel_map_align(self.h, points_ptr, int(n), _p(q), C.byref(prm), _p(out), C.byref(res)), "svo_voxel_map_align")
        return out, _align_result(res)

    def normals(self, normals_ptr, params=None, counts_ptr=None, **overrides):
        """svo_voxel_map_normals_dev: a normal and a curvature per slot from the means of the 27 voxels around it, into the
        voxel_map_normals_bytes(self.params) bytes at the device pointer normals_ptr (16-byte aligned, one VoxelNormal per slot,
        indexed by slot; {0, 0, 0, -1}: no normal).  counts_ptr: 8 uint64 on the device (NORMALS_COUNTS, then zeros), or None.
        params: a VoxelNormalsParams and / or its fields as keywords.  Nothing in the map changes; run it again after inserts,
        removals or a carve.  Asynchronous on the context's stream."""
        prm = _params(voxel_normals_default_params, params, **overrides)
        self.ctx._chk(self.L.svo_voxel_map_normals_dev(self.h, C.byref(prm), normals_ptr, counts_ptr), "svo_voxel_map_normals_dev")

    def normals_host(self, params=None, **overrides):
        """svo_voxel_map_normals: normals() into memory of its own, synchronous.  Returns (a VoxelNormal array with one record per
        slot, {"n_centres", "n_valid", "n_few", "n_collinear", "n_curved"})."""
        prm = _params(voxel_normals_default_params, params, **overrides)
        out, c = np.empty(self.capacity, VoxelNormal), np.zeros(VOXEL_NORMALS_COUNTS, np.uint64)
        self.ctx._chk(self.L.svo_voxel_map_normals(self.h, C.byref(prm), _p(out), _p(c)), "svo_voxel_map_normals")
        return out, dict(zip(NORMALS_COUNTS, (int(v) for v in c)))

    def align_plane_sums(self, normals_ptr, points_ptr, n, c2w12=None, pose7=None, params=None, sums_ptr=None, **overrides):
        """svo_voxel_map_align_plane_sums_dev / _pose7_dev: align_sums' matching, then the normal equations of the point-to-plane
        increment along the matched voxel's normal (normals_ptr: what normals() wrote) and the five counts, into the 40 int64 at
        the device pointer sums_ptr (include/svo.h, "Voxel map align, plane form").  Asynchronous on the context's stream."""
        prm = _params(lambda: voxel_align_default_params(self.params.voxel_size), params, **overrides)
        self._by_pose("align_plane_sums", "c2w12", c2w12, pose7, "align_plane_sums", (normals_ptr, points_ptr, int(n)), (C.byref(prm), sums_ptr))

    def align_plane(self, normals_ptr, points_ptr, n, pose7, params=None, **overrides):
        """svo_voxel_map_align_plane: align() with the point-to-plane residual; synchronous.  Run normals() after the map's last
        change and before this.  Returns (pose7_out, the result dict of align(): the costs are word 28, the matches word 29)."""
        prm = _params(lambda: voxel_align_default_params(self.params.voxel_size), params, **overrides)
        q = _f64(pose7).reshape(7)
        out, res = np.empty(7, np.float64), VoxelAlignResult()
        self.ctx._chk(self.L.svo_voxel_map_align_plane(self.h, normals_ptr, points_ptr, int(n), _p(q), C.byref(prm), _p(out), C.byref(res)),
                      "svo_voxel_map_align_plane")
        return out, _align_result(res)

    def occupancy(self, bits_ptr, origin, dims, min_count=1, counts_ptr=None):
        """svo_voxel_map_occupancy_dev: the dense bit volume of the map's voxels with at least min_count points, dims = (d0, d1, d2)
        voxels from the voxel indices origin, into the voxel_occupancy_bytes(dims) bytes at the device pointer bits_ptr (8-byte
        aligned): voxel i is bit j_0 + d0 (j_1 + d1 j_2), j = i - origin, of little-endian u64 words.  counts_ptr: 2 uint32 on the
        device (OCCUPANCY_COUNTS).  Nothing in the map changes.  Asynchronous on the context's stream."""
        self.ctx._chk(self.L.svo_voxel_map_occupancy_dev(self.h, int(min_count), _p(_int3(origin)), _p(_int3(dims)), bits_ptr, counts_ptr),
                      "svo_voxel_map_occupancy_dev")

    def occupancy_host(self, origin, dims, min_count=1):
        """svo_voxel_map_occupancy: occupancy() into memory of its own, synchronous.  Returns (the volume's uint64 words,
        {"n_inside", "n_outside"})."""
        bits, c = np.empty(voxel_occupancy_bytes(dims) // 8, np.uint64), np.zeros(2, np.uint32)
        self.ctx._chk(self.L.svo_voxel_map_occupancy(self.h, int(min_count), _p(_int3(origin)), _p(_int3(dims)), _p(bits), _p(c)), "svo_voxel_map_occupancy")
        return bits, dict(zip(OCCUPANCY_COUNTS, (int(v) for v in c)))

    def locate_scores(self, bits_ptr, origin, dims, points_ptr, n, mats, box, hits_ptr=None, best_ptr=None):
        """svo_voxel_map_locate_scores_dev: for each of the K camera->world matrices mats (K x 12 doubles, K <= 63) and every
        whole-voxel shift |s_r| <= box_r (<= 16), how many of the n records land in a set bit of the volume occupancy() wrote:
        K * S0 * S1 * S2 uint32 at the device pointer hits_ptr and K VoxelLocateBest records at best_ptr (include/svo.h, "Voxel map
        locate").  Asynchronous on the context's stream."""
        m = _f64(mats).reshape(-1, 12)
        self.ctx._chk(self.L.svo_voxel_map_locate_scores_dev(self.h, bits_ptr, _p(_int3(origin)), _p(_int3(dims)), points_ptr, int(n), _p(m), len(m),
                                                             _p(_int3(box)), hits_ptr, best_ptr), "svo_voxel_map_locate_scores_dev")

    def locate(self, points_ptr, n, pose7, params=None, align_params=None, normals_ptr=None, workspace_ptr=None, **overrides):
        """svo_voxel_map_locate: search a box of whole-voxel shifts and a fan of turns about one world axis for the cloud's pose, then
        refine the best candidates with align() (align_plane() if normals_ptr is given); synchronous.  workspace_ptr: a device
        pointer, 256-byte aligned, voxel_locate_workspace_bytes(params) bytes.  params: a VoxelLocateParams and / or its fields as
        keywords; align_params: a VoxelAlignParams (default: voxel_align_default_params).  Locate BEFORE inserting the cloud.
        Returns (pose7_out, {"status", "k", "shift", "hits", "rank", "n_refined", "coarse_pose7", "align"})."""
        threes = {k: overrides.pop(k) for k in ("box", "dims") if overrides.get(k) is not None}
        prm = _params(lambda: voxel_locate_default_params(self.params.voxel_size), params, **overrides)
        for k, v in threes.items():
            setattr(prm, k, (C.c_int * 3)(*(int(x) for x in v)))
        ap = _params(lambda: voxel_align_default_params(self.params.voxel_size), align_params)
        q = _f64(pose7).reshape(7)
        out, res = np.empty(7, np.float64), VoxelLocateResult()
        self.ctx._chk(self.L.svo_voxel_map_locate(self.h, normals_ptr, points_ptr, int(n), _p(q), C.byref(prm), C.byref(ap), workspace_ptr, _p(out),
                                                  C.byref(res)), "svo_voxel_map_locate")
        return out, {"status": VOXEL_LOCATE_STATUS[res.status], "k": res.k, "shift": tuple(res.shift), "hits": int(res.hits), "rank": res.rank,
                     "n_refined": res.n_refined, "coarse_pose7": np.array(list(res.coarse_pose7), np.float64), "align": _align_result(res.align)}

    def occupancy_coarse(self, bits_ptr, dims, coarse_ptr):
        """svo_voxel_occupancy_coarse_dev: one bit per 8 x 8 x 8 block of the volume occupancy() wrote at bits_ptr, set iff any of the
        block's voxels is, into the voxel_occupancy_coarse_bytes(dims) bytes at the device pointer coarse_ptr (8-byte aligned).  Run
        it after occupancy() and before rays() / raycast() with coarse_ptr.  Asynchronous on the context's stream."""
        self.ctx._chk(self.L.svo_voxel_occupancy_coarse_dev(self.h, bits_ptr, _p(_int3(dims)), coarse_ptr), "svo_voxel_occupancy_coarse_dev")

    def rays(self, bits_ptr, origin, dims, rays_ptr, n, hits_ptr=None, coarse_ptr=None, min_step=1, counts_ptr=None):
        """svo_voxel_occupancy_rays_dev: what each of the n VoxelRay records at the device pointer rays_ptr (16-byte aligned, world
        metres) meets first in the volume occupancy() wrote: n VoxelRayHit records at hits_ptr (16-byte aligned) and 6 uint64
        RAYS_COUNTS at counts_ptr (or None).  coarse_ptr: what occupancy_coarse() wrote (the block-skipping walk), or None (the
        plain walk); the same bytes either way (include/svo.h, "Voxel map sight lines").  Asynchronous on the context's stream."""
        self.ctx._chk(self.L.svo_voxel_occupancy_rays_dev(self.h, bits_ptr, coarse_ptr, _p(_int3(origin)), _p(_int3(dims)), rays_ptr, int(n), int(min_step),
                                                          hits_ptr, counts_ptr), "svo_voxel_occupancy_rays_dev")

    def rays_host(self, bits_ptr, origin, dims, rays, coarse_ptr=None, min_step=1):
        """svo_voxel_occupancy_rays: rays() for a host array of VoxelRay records, synchronous; bits_ptr and coarse_ptr stay device
        pointers.  Returns (a VoxelRayHit array, {"n_hit", "n_left", "n_range", "n_outside", "n_rejected", "n_steps"})."""
        r = np.ascontiguousarray(rays, dtype=VoxelRay)
        out, c = np.empty(max(len(r), 1), VoxelRayHit), np.zeros(6, np.uint64)
        self.ctx._chk(self.L.svo_voxel_occupancy_rays(self.h, bits_ptr, coarse_ptr, _p(_int3(origin)), _p(_int3(dims)), _p(r) if len(r) else None, len(r),
                                                      int(min_step), _p(out), _p(c)), "svo_voxel_occupancy_rays")
        return out[:len(r)], dict(zip(RAYS_COUNTS, (int(v) for v in c)))

    def raycast(self, bits_ptr, origin, dims, width, height, cam, c2w12=None, pose7=None, params=None, coarse_ptr=None, disp_ptr=None,
                cell_ptr=None, counts_ptr=None, **overrides):
        """svo_voxel_occupancy_raycast_dev / _pose7_dev: one ray per pixel of `cam` at the pose, exactly one of c2w12 (3 x 4
        camera->world) and pose7, walked through the volume at bits_ptr: a tight CV_16S disparity map in sixteenths at disp_ptr
        (FILTERED = -16 where the ray meets nothing), the hit voxel's bit number per pixel at cell_ptr (uint32, or None) and 7
        uint64 RAYCAST_COUNTS at counts_ptr (or None).  params: a VoxelRaycastParams and / or its fields as keywords; coarse_ptr as
        in rays().  A view without the splat render's holes, in the format carve() takes.  Asynchronous on the context's stream."""
        if (c2w12 is None) == (pose7 is None):
            raise ValueError("VoxelMap.raycast: give exactly one of c2w12 and pose7")
        prm = _params(voxel_raycast_default_params, params, **overrides)
        fn, a = ("svo_voxel_occupancy_raycast_dev", _f64(c2w12).reshape(12)) if pose7 is None else ("svo_voxel_occupancy_raycast_pose7_dev", _f64(pose7).reshape(7))
        self.ctx._chk(getattr(self.L, fn)(self.h, bits_ptr, coarse_ptr, _p(_int3(origin)), _p(_int3(dims)), int(width), int(height), C.byref(cam), _p(a),
                                          C.byref(prm), disp_ptr, cell_ptr, counts_ptr), fn)

    def raycast_host(self, width, height, cam, c2w12=None, pose7=None, dims=(512, 128, 512), min_count=1, params=None, **overrides):
        """svo_voxel_map_raycast: the occupancy volume of dims voxels around the camera centre, its coarse volume and raycast() in one
        synchronous call that allocates and frees.  Returns (disp16 (height, width) int16, cell (height, width) uint32,
        {RAYCAST_COUNTS..., "origin": the volume's origin})."""
        if (c2w12 is None) == (pose7 is None):
            raise ValueError("VoxelMap.raycast_host: give exactly one of c2w12 and pose7")
        prm = _params(voxel_raycast_default_params, params, **overrides)
        m = _f64(pose7_to_cam_to_world(pose7) if c2w12 is None else c2w12).reshape(12)
        d = np.empty((max(int(height), 1), max(int(width), 1)), np.int16)
        cell, c, o = np.empty(d.shape, np.uint32), np.zeros(7, np.uint64), np.zeros(3, np.int32)
        self.ctx._chk(self.L.svo_voxel_map_raycast(self.h, int(min_count), _p(_int3(dims)), int(width), int(height), C.byref(cam), _p(m), C.byref(prm), _p(d),
                                                   _p(cell), _p(c), _p(o)), "svo_voxel_map_raycast")
        counts = dict(zip(RAYCAST_COUNTS, (int(v) for v in c)))
        counts["origin"] = tuple(int(v) for v in o)
        return d, cell, counts

    def _distance_params(self, params, overrides):
        return _params(lambda: voxel_distance_default_params(self.params.voxel_size), params, **overrides)

    def distance(self, bits_ptr, dims, params=None, workspace_ptr=None, dist2_ptr=None, nearest_ptr=None, clearance_ptr=None, inflated_ptr=None,
                 counts_ptr=None, **overrides):
        """svo_voxel_occupancy_distance_dev: per cell of the volume occupancy() wrote at bits_ptr the exact squared distance in voxels
        to the nearest set bit, capped at max_dist (uint16 at dist2_ptr, 0xFFFF beyond), and optionally that bit's number (uint32 at
        nearest_ptr), the distance in map units (float32 at clearance_ptr), the volume inflated by inflate_radius in the occupancy's
        bit format (inflated_ptr; rays() over it is a swept-sphere test) and 4 uint64 DISTANCE_COUNTS at counts_ptr.  workspace_ptr:
        voxel_distance_workspace_bytes(dims, nearest_ptr is not None) device bytes, 8-byte aligned.  params: a VoxelDistanceParams and
        / or its fields as keywords.  Run it after occupancy().  Asynchronous on the context's stream."""
        prm = self._distance_params(params, overrides)
        out = VoxelDistanceOut(dist2_ptr, nearest_ptr, clearance_ptr, inflated_ptr)
        self.ctx._chk(self.L.svo_voxel_occupancy_distance_dev(self.h, bits_ptr, _p(_int3(dims)), C.byref(prm), workspace_ptr, C.byref(out), counts_ptr),
                      "svo_voxel_occupancy_distance_dev")

    def distance_host(self, origin, dims, min_count=1, params=None, nearest=True, clearance=True, inflated=True, **overrides):
        """svo_voxel_map_distance: occupancy() and distance() into memory of its own, synchronous; allocates and frees.  Returns a
        dict: "dist2" (d2, d1, d0) uint16, and where asked "nearest" uint32, "clearance" float32 of that shape and "inflated", the
        volume's uint64 words; "counts": {DISTANCE_COUNTS...}."""
        prm = self._distance_params(params, overrides)
        d = _int3(dims)
        shape = (max(int(d[2]), 1), max(int(d[1]), 1), max(int(d[0]), 1))
        res = {"dist2": np.empty(shape, np.uint16)}
        if nearest:
            res["nearest"] = np.empty(shape, np.uint32)
        if clearance:
            res["clearance"] = np.empty(shape, np.float32)
        if inflated:
            res["inflated"] = np.empty(max(shape[0] * shape[1] * shape[2] // 64, 1), np.uint64)
        out = VoxelDistanceOut(*(res[k].ctypes.data if k in res else None for k in ("dist2", "nearest", "clearance", "inflated")))
        c = np.zeros(4, np.uint64)
        self.ctx._chk(self.L.svo_voxel_map_distance(self.h, int(min_count), _p(_int3(origin)), _p(d), C.byref(prm), C.byref(out), _p(c)), "svo_voxel_map_distance")
        res["counts"] = dict(zip(DISTANCE_COUNTS, (int(v) for v in c)))
        return res

    def distance_query(self, dist2_ptr, origin, dims, spheres_ptr, n, hits_ptr=None, counts_ptr=None):
        """svo_voxel_distance_query_dev: for each of the n VoxelSphere records at the device pointer spheres_ptr (16-byte aligned, world
        metres) the cell of its centre, that cell's dist2 and clearance in the field distance() wrote at dist2_ptr, and whether a
        sphere of its radius collides (cell centre to cell centre; add sqrt(3) * voxel_size to the radius for a conservative test):
        n VoxelSphereHit records at hits_ptr (16-byte aligned) and 6 uint64 DISTANCE_QUERY_COUNTS at counts_ptr (or None).
        Asynchronous on the context's stream."""
        self.ctx._chk(self.L.svo_voxel_distance_query_dev(self.h, dist2_ptr, _p(_int3(origin)), _p(_int3(dims)), spheres_ptr, int(n), hits_ptr, counts_ptr),
                      "svo_voxel_distance_query_dev")

    def distance_query_host(self, dist2_ptr, origin, dims, spheres):
        """svo_voxel_distance_query: distance_query() for a host array of VoxelSphere records, synchronous; dist2_ptr stays a device
        pointer.  Returns (a VoxelSphereHit array, {DISTANCE_QUERY_COUNTS...})."""
        s = np.ascontiguousarray(spheres, dtype=VoxelSphere)
        out, c = np.empty(max(len(s), 1), VoxelSphereHit), np.zeros(6, np.uint64)
        self.ctx._chk(self.L.svo_voxel_distance_query(self.h, dist2_ptr, _p(_int3(origin)), _p(_int3(dims)), _p(s) if len(s) else None, len(s), _p(out), _p(c)),
                      "svo_voxel_distance_query")
        return out[:len(s)], dict(zip(DISTANCE_QUERY_COUNTS, (int(v) for v in c)))

    def _route_params(self, params, overrides):
        return _params(lambda: voxel_route_default_params(self.params.voxel_size), params, **overrides)

    def route(self, closed_ptr, dims, goals_ptr, n_goals, params=None, dist2_ptr=None, starts_ptr=None, n_starts=0, workspace_ptr=None, cost_ptr=None,
              next_ptr=None, path_ptr=None, path_len_ptr=None, path_status_ptr=None, counts_ptr=None, **overrides):
        """svo_voxel_occupancy_route_dev: the cost-to-go field to the goal cells through the free space of the bit volume behind
        closed_ptr (the occupancy's layout, a cell passable iff its bit is 0: distance()'s inflated or occupancy()'s bits), the first
        move per cell (26 neighbours) and the paths from the start cells.  params (a VoxelRouteParams) and / or its fields as keywords.
        All pointers are the caller's device memory: dist2_ptr distance()'s uint16 field or None, goals_ptr n_goals and starts_ptr
        n_starts uint32 cell numbers (voxel_occupancy_cell_of), workspace_ptr voxel_route_workspace_bytes(dims) bytes, cost_ptr one
        uint32 per cell (required), next_ptr one uint8 per cell, path_ptr n_starts x max_path uint32, path_len_ptr uint32 and
        path_status_ptr uint8 per start (the three together or None), counts_ptr 8 uint64 (VOXEL_ROUTE_COUNTS and two zeros) or None.
        Asynchronous on the context's stream."""
        prm = self._route_params(params, overrides)
        out = VoxelRouteOut(cost_ptr, next_ptr, path_ptr, path_len_ptr, path_status_ptr)
        self.ctx._chk(self.L.svo_voxel_occupancy_route_dev(self.h, closed_ptr, _p(_int3(dims)), dist2_ptr, C.byref(prm), goals_ptr, int(n_goals), starts_ptr,
                                                           int(n_starts), workspace_ptr, C.byref(out), counts_ptr), "svo_voxel_occupancy_route_dev")

    def route_host(self, closed_ptr, dims, goals, starts=None, dist2_ptr=None, params=None, **overrides):
        """svo_voxel_occupancy_route: route() with host goals and starts and host results, synchronous; closed_ptr and dist2_ptr stay
        device pointers.  Returns {"cost" (d2, d1, d0) uint32 with VOXEL_ROUTE_NONE, "next" (d2, d1, d0) uint8, "counts"
        {VOXEL_ROUTE_COUNTS}} and, with starts, "path" (n_starts, max_path) uint32 (VOXEL_ROUTE_NONE where nothing was written),
        "path_len" uint32 and "path_status" uint8 per start."""
        prm = self._route_params(params, overrides)
        d = _int3(dims)
        shape = (max(int(d[2]), 1), max(int(d[1]), 1), max(int(d[0]), 1))
        goals = np.ascontiguousarray(goals, np.uint32).ravel()
        starts = None if starts is None else np.ascontiguousarray(starts, np.uint32).ravel()
        ns = 0 if starts is None else len(starts)
        res = {"cost": np.empty(shape, np.uint32), "next": np.full(shape, 255, np.uint8)}
        if ns:
            if not 1 <= prm.max_path <= 1 << 20:
                raise SvoError("svo_voxel_occupancy_route: voxel_route: max_path outside 1..2^20")
            res.update(path=np.full((ns, prm.max_path), VOXEL_ROUTE_NONE, np.uint32), path_len=np.zeros(ns, np.uint32), path_status=np.zeros(ns, np.uint8))
        out = VoxelRouteOut(*(res[k].ctypes.data if k in res else None for k in ("cost", "next", "path", "path_len", "path_status")))
        c = np.zeros(8, np.uint64)
        self.ctx._chk(self.L.svo_voxel_occupancy_route(self.h, closed_ptr, _p(d), dist2_ptr, C.byref(prm), _p(goals) if len(goals) else None, len(goals),
                                                       _p(starts) if ns else None, ns, C.byref(out), _p(c)), "svo_voxel_occupancy_route")
        res["counts"] = dict(zip(VOXEL_ROUTE_COUNTS, (int(v) for v in c)))
        return res

    def insert_keyframe_clouds(self, table, poses7):
        """The list Pipeline.keyframe_clouds() / PipelineGroup.keyframe_clouds() returns, one pose7 per entry: every entry's device
        cloud is inserted from its "dev" pointer (no host copy).  Call before the next process call replaces the clouds."""
        if len(table) != len(poses7):
            raise ValueError("VoxelMap.insert_keyframe_clouds: one pose7 per table entry")
        for e, q in zip(table, poses7):
            self.insert(e["dev"], e["n_stored"], pose7=q)

    def carve(self, disp_ptr, width, height, cam, w2c12=None, pose7=None, params=None, radius=None, margin16=None, keep_count=None,
              counts_ptr=None):
        """svo_voxel_map_carve_dev / _pose7_dev: the voxels the keyframe whose tight CV_16S map sits at the device pointer saw through
        lose their payload (the key stays).  Exactly one of w2c12 (3 x 4 world->camera) and pose7; counts_ptr: 3 uint64 on the
        device {n_live, n_tested, n_carved}, or None.  Asynchronous on the context's stream."""
        prm = _carve_params(params, radius, margin16, keep_count)
        self._by_pose("carve", "w2c12", w2c12, pose7, "carve", (disp_ptr, int(width), int(height), C.byref(cam)), (C.byref(prm), counts_ptr))

    def carve_host(self, disp16, cam, w2c12=None, pose7=None, params=None, radius=None, margin16=None, keep_count=None):
        """svo_voxel_map_carve: disp16 a (height, width) int16 numpy map; synchronous.  Returns {"n_live", "n_tested", "n_carved"}."""
        d = np.ascontiguousarray(disp16, np.int16)
        if d.ndim != 2:
            raise ValueError("VoxelMap.carve_host: disp16 must be a (height, width) map")
        prm = _carve_params(params, radius, margin16, keep_count)
        c = np.zeros(3, np.uint64)
        self._by_pose("carve_host", "w2c12", w2c12, pose7, "carve", (_p(d), d.shape[1], d.shape[0], C.byref(cam)), (C.byref(prm), _p(c)),
                      pose7_to_world_to_cam)
        return {"n_live": int(c[0]), "n_tested": int(c[1]), "n_carved": int(c[2])}

    def copy_live_to(self, dst, min_count=1, box=None):
        """svo_voxel_map_copy_live_dev: every voxel with count >= min_count (inside box = (lo_xyz, hi_xyz) in map units, if given) is
        added to dst: a fresh dst gives the map without its carved slots, a non-empty one a merge.  Asynchronous."""
        b = None if box is None else _f64(np.asarray(box, np.float64)).reshape(6)
        self.ctx._chk(self.L.svo_voxel_map_copy_live_dev(self.h, dst.h, int(min_count), _p(b)), "svo_voxel_map_copy_live_dev")

    def render(self, width, height, cam, w2c12=None, pose7=None, params=None, min_count=None, max_radius=None, workspace_ptr=None,
               disp_ptr=None, intensity_ptr=None, counts_ptr=None):
        """svo_voxel_map_render_dev / _pose7_dev: the map seen by `cam` at the pose, exactly one of w2c12 (3 x 4 world->camera) and
        pose7.  All pointers are the caller's device memory, as everywhere in this class: workspace_ptr
        voxel_render_workspace_bytes(width, height) bytes, disp_ptr width * height int16, intensity_ptr as many uint8 or None,
        counts_ptr 4 uint64 {n_qualifying, n_drawn, n_splat, n_pixels} or None.  Asynchronous on the context's stream; returns
        {"disp16", "intensity", "counts", "workspace", "width", "height"}: the pointers the outputs are behind once the stream
        reaches this point."""
        prm = _render_params(params, min_count, max_radius)
        self._by_pose("render", "w2c12", w2c12, pose7, "render", (int(width), int(height), C.byref(cam)),
                      (C.byref(prm), workspace_ptr, disp_ptr, intensity_ptr, counts_ptr))
        return {"disp16": disp_ptr, "intensity": intensity_ptr, "counts": counts_ptr, "workspace": workspace_ptr,
                "width": int(width), "height": int(height)}

    def render_host(self, width, height, cam, w2c12=None, pose7=None, params=None, min_count=None, max_radius=None):
        """svo_voxel_map_render: synchronous.  Returns (disp16 (height, width) int16 with FILTERED = -16 where nothing is seen,
        intensity (height, width) uint8, {"n_qualifying", "n_drawn", "n_splat", "n_pixels"})."""
        prm = _render_params(params, min_count, max_radius)
        d = np.empty((max(int(height), 1), max(int(width), 1)), np.int16)
        g = np.empty(d.shape, np.uint8)
        c = np.zeros(4, np.uint64)
        self._by_pose("render_host", "w2c12", w2c12, pose7, "render", (int(width), int(height), C.byref(cam)), (C.byref(prm), _p(d), _p(g), _p(c)),
                      pose7_to_world_to_cam)
        return d, g, {"n_qualifying": int(c[0]), "n_drawn": int(c[1]), "n_splat": int(c[2]), "n_pixels": int(c[3])}

    def render_set_mode(self, cooperative=True, precheck=False):
        """svo_voxel_render_set_mode (measurement aid): how the splat launch draws; no bit of a render depends on it."""
        self.ctx._chk(self.L.svo_voxel_render_set_mode(self.h, int(bool(cooperative)), int(bool(precheck))), "svo_voxel_render_set_mode")

    def grid(self, params=None, workspace_ptr=None, cls_ptr=None, top_ptr=None, bottom_ptr=None, intensity_ptr=None, n_voxels_ptr=None,
             n_points_ptr=None, counts_ptr=None, **overrides):
        """svo_voxel_map_grid_dev: the map's ground plan, na x nb cells over two of its axes.  params (a VoxelGridParams; None: the
        defaults for this map's voxel size) and / or its fields as keywords.  All pointers are the caller's device memory:
        workspace_ptr voxel_grid_workspace_bytes(na, nb) bytes, cls_ptr na * nb uint8 (required), top_ptr / bottom_ptr float32,
        intensity_ptr uint8, n_voxels_ptr uint32, n_points_ptr uint64 or None each, counts_ptr 5 uint64 GRID_COUNTS or None.
        Asynchronous on the context's stream; returns {"cls", "top", "bottom", "intensity", "n_voxels", "n_points", "counts",
        "workspace", "na", "nb"}: the pointers the outputs are behind once the stream reaches this point."""
        prm = _grid_params(self.params.voxel_size, params, overrides)
        out = VoxelGridOut(cls_ptr, top_ptr, bottom_ptr, intensity_ptr, n_voxels_ptr, n_points_ptr)
        self.ctx._chk(self.L.svo_voxel_map_grid_dev(self.h, C.byref(prm), workspace_ptr, C.byref(out), counts_ptr), "svo_voxel_map_grid_dev")
        return {"cls": cls_ptr, "top": top_ptr, "bottom": bottom_ptr, "intensity": intensity_ptr, "n_voxels": n_voxels_ptr,
                "n_points": n_points_ptr, "counts": counts_ptr, "workspace": workspace_ptr, "na": prm.na, "nb": prm.nb}

    def grid_host(self, params=None, **overrides):
        """svo_voxel_map_grid: synchronous.  Returns (cls (na, nb) uint8 of VOXEL_GRID_UNKNOWN / LEVEL / OBSTACLE, top and bottom
        (na, nb) float32 (-inf / +inf where unknown), intensity uint8, n_voxels uint32, n_points uint64, {GRID_COUNTS})."""
        prm = _grid_params(self.params.voxel_size, params, overrides)
        shape = (max(prm.na, 1), max(prm.nb, 1))
        arrays = [np.empty(shape, t) for t in (np.uint8, np.float32, np.float32, np.uint8, np.uint32, np.uint64)]
        out = VoxelGridOut(*(a.ctypes.data for a in arrays))
        c = np.zeros(5, np.uint64)
        self.ctx._chk(self.L.svo_voxel_map_grid(self.h, C.byref(prm), C.byref(out), _p(c)), "svo_voxel_map_grid")
        return (*arrays, dict(zip(GRID_COUNTS, (int(v) for v in c))))

    def grid_set_mode(self, precheck=None):
        """svo_voxel_grid_set_mode (measurement aid): whether a load skips the walk's max atomics where it can; no bit of a grid depends
        on it.  None: the library's default."""
        self.ctx._chk(self.L.svo_voxel_grid_set_mode(self.h, int(GRID_PRECHECK_DEFAULT if precheck is None else bool(precheck))), "svo_voxel_grid_set_mode")

    def stats(self):
        """The four counters as a dict (synchronises)."""
        s = VoxelMapStats()
        self.ctx._chk(self.L.svo_voxel_map_stats(self.h, C.byref(s)), "svo_voxel_map_stats")
        return {"n_voxels": int(s.n_voxels), "n_inserted": int(s.n_inserted), "n_rejected": int(s.n_rejected), "n_dropped": int(s.n_dropped)}

    def extract_dev(self, min_count, points_ptr, max_points, counts_ptr):
        """svo_voxel_map_extract_dev: raw device pointers (ints); counts_ptr: 2 int32 {n_total, n_stored}.  Asynchronous."""
        self.ctx._chk(self.L.svo_voxel_map_extract_dev(self.h, int(min_count), points_ptr, int(max_points), counts_ptr),
                      "svo_voxel_map_extract_dev")

    def extract(self, min_count=1, max_points=None):
        """(points as a CLOUD_POINT_DTYPE array of n_stored records in no defined order, n_total).  max_points None: all of them."""
        nt, ns = C.c_int(0), C.c_int(0)
        if max_points is None:  # count first: the table may be far larger than the map
            self.ctx._chk(self.L.svo_voxel_map_extract(self.h, int(min_count), None, 0, C.byref(nt), C.byref(ns)), "svo_voxel_map_extract")
            max_points = nt.value
        pts = np.empty(max(int(max_points), 1), CLOUD_POINT_DTYPE)
        self.ctx._chk(self.L.svo_voxel_map_extract(self.h, int(min_count), _p(pts), int(max_points), C.byref(nt), C.byref(ns)),
                      "svo_voxel_map_extract")
        return pts[:ns.value].copy(), nt.value

    def download(self):
        """The table as a dict of numpy uint64 arrays of `capacity` entries: "keys" (EMPTY = 2^64 - 1), "ci" (count << 40 | intensity
        sum), "sx", "sy", "sz"."""
        buf = np.empty((5, self.capacity), np.uint64)
        self.ctx._chk(self.L.svo_voxel_map_download(self.h, _p(buf), buf.nbytes), "svo_voxel_map_download")
        return {k: buf[i] for i, k in enumerate(("keys", "ci", "sx", "sy", "sz"))}


class VoxelLedger:
    """svo_voxel_ledger: the clouds of the keyframes still in the window, held on the device with the pose each was inserted under
    (include/svo.h, "voxel map ledger").  insert each new keyframe, update the held ones when newer poses exist, retire one when it
    leaves the window, carve only after updating.  Close it before its map."""

    def __init__(self, vmap, max_keyframes, max_points):
        self.map, self.ctx, self.L = vmap, vmap.ctx, vmap.L
        self.params = VoxelLedgerParams(int(max_keyframes), int(max_points))
        self.h = C.c_void_p()
        self.ctx._chk(self.L.svo_voxel_ledger_create(vmap.h, C.byref(self.params), C.byref(self.h)), "svo_voxel_ledger_create")

    def close(self):
        if self.h:
            if self.map.h and self.ctx.h:
                self.L.svo_voxel_ledger_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def insert(self, id, dev_ptr, n, pose7):
        """The n records at the device pointer are copied into the ledger and the copy is inserted into the map under pose7."""
        q = _f64(pose7).reshape(7)
        self.ctx._chk(self.L.svo_voxel_ledger_insert_pose7_dev(self.h, int(id), dev_ptr, int(n), _p(q)), "svo_voxel_ledger_insert_pose7_dev")

    def update(self, id, pose7, counts_ptr=None):
        """The held cloud moves from the pose it was last inserted under to pose7 (nothing is launched when the matrices agree)."""
        q = _f64(pose7).reshape(7)
        self.ctx._chk(self.L.svo_voxel_ledger_update_pose7(self.h, int(id), _p(q), counts_ptr), "svo_voxel_ledger_update_pose7")

    def update_all(self, poses7):
        """{id: pose7}: update() of each, in ascending id order."""
        for k in sorted(poses7):
            self.update(k, poses7[k])

    def retire(self, id):
        """The pose is final: the map keeps the cloud, the slot is free."""
        self.ctx._chk(self.L.svo_voxel_ledger_retire(self.h, int(id)), "svo_voxel_ledger_retire")

    def remove(self, id, counts_ptr=None):
        """The held cloud is taken out of the map and the slot is free."""
        self.ctx._chk(self.L.svo_voxel_ledger_remove(self.h, int(id), counts_ptr), "svo_voxel_ledger_remove")

    def ids(self):
        """The held ids, ascending."""
        out = np.zeros(self.params.max_keyframes, np.int64)
        n = C.c_int(0)
        self.ctx._chk(self.L.svo_voxel_ledger_ids(self.h, _p(out), len(out), C.byref(n)), "svo_voxel_ledger_ids")
        return [int(v) for v in out[:n.value]]

    def get(self, id):
        """{"pose7", "n", "dev"}: the recorded pose, the record count and the device pointer of the held copy."""
        q = np.zeros(7, np.float64)
        n, dev = C.c_int(0), C.c_void_p()
        self.ctx._chk(self.L.svo_voxel_ledger_get(self.h, int(id), _p(q), C.byref(n), C.byref(dev)), "svo_voxel_ledger_get")
        return {"pose7": q, "n": n.value, "dev": dev.value or 0}


class BA:
    """svo_ba wrapper: sliding-window graph (add_keyframe / solve) and the bulk-problem interface."""

    def __init__(self, ctx, window_size, focal, cx, cy, baseline=0.0, max_landmarks=1 << 16,
                 max_observations=1 << 18, max_iterations=50, max_time_s=0.0, max_features=400, accumulation="auto", device_lm=None, bulk_control=None, solve_form=None):
        self.ctx = ctx
        self.L = ctx.L
        cam = CameraInfo(focal, cx, cy, 0, 0, 0, 0, baseline)
        opt = BAOptions()
        self.L.svo_ba_default_options(C.byref(opt))
        opt.max_iterations = max_iterations
        opt.max_time_s = max_time_s
        opt.max_features = max_features
        opt.accumulation = BA_ACC[accumulation]
        self.h = C.c_void_p()
        ctx._chk(self.L.svo_ba_create(ctx.h, C.byref(self.h), window_size, C.byref(cam), C.byref(opt),
                                      max_landmarks, max_observations), "svo_ba_create")
        if device_lm is not None:
            ctx._chk(self.L.svo_ba_set_device_lm(self.h, 1 if device_lm else 0), "svo_ba_set_device_lm")
        if solve_form is not None:  # "wide" / "compact": which device-resident form a window solve takes
            ctx._chk(self.L.svo_ba_set_solve_form(self.h, {"wide": 0, "compact": 1}[solve_form]), "svo_ba_set_solve_form")
        if bulk_control is not None:  # bulk / sharded solves: step control on the device (True) or host-driven (False)
            ctx._chk(self.L.svo_ba_set_bulk_control(self.h, 1 if bulk_control else 0), "svo_ba_set_bulk_control")
        self.L.svo_ba_destroy.argtypes = [C.c_void_p]
        self._cb = None

    def close(self):
        if self.h:
            self.L.svo_ba_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def load_problem(self, poses7, points3, obs_pose, obs_point, obs_uv):
        poses7, points3, obs_uv = _f64(poses7), _f64(points3), _f64(obs_uv)
        op = np.ascontiguousarray(obs_pose, np.int32)
        oj = np.ascontiguousarray(obs_point, np.int32)
        self._shape = (poses7.shape[0], points3.shape[0])
        self.ctx._chk(self.L.svo_ba_load_problem(self.h, poses7.shape[0], _p(poses7), points3.shape[0],
                                                 _p(points3), op.shape[0], _p(op), _p(oj), _p(obs_uv)),
                      "svo_ba_load_problem")

    def set_allreduce(self, fn):
        """fn(dev_ptr:int, n_doubles:int) -> 0; must sum the device buffer in place over all ranks."""
        self._cb = ALLREDUCE_FN(lambda ptr, n, user: int(fn(ptr, n) or 0)) if fn else None
        self.ctx._chk(self.L.svo_ba_set_allreduce(self.h, self._cb if self._cb else C.cast(None, ALLREDUCE_FN), None),
                      "svo_ba_set_allreduce")

    def set_comm(self, nccl_comm):
        """nccl_comm: ncclComm_t as an int / c_void_p (see rccl_comm_create); None detaches."""
        self.ctx._chk(self.L.svo_ba_set_comm(self.h, C.c_void_p(nccl_comm) if nccl_comm else None), "svo_ba_set_comm")

    def solve_problem(self):
        s = BASummary()
        self.ctx._chk(self.L.svo_ba_solve_problem(self.h, C.byref(s)), "svo_ba_solve_problem")
        return s

    def set_wave_chunks(self, k):
        """Chunks per wavefront of this adjuster's wide device-resident solves (1 .. svo_ba_wave_chunks_limit(); 0: the process default,
        raised by the admission where its budget asks for it)."""
        self.ctx._chk(self.L.svo_ba_set_wave_chunks(self.h, int(k)), "svo_ba_set_wave_chunks")

    def solve_forms(self):
        """([compact solves, wide solves at k = 1, 2, ... chunks per wavefront], solves that gave up and were run again) of this adjuster so far."""
        n = self.L.svo_ba_wave_chunks_limit() + 1
        out, gu = (C.c_long * n)(), C.c_long(0)
        self.ctx._chk(self.L.svo_ba_solve_forms(self.h, out, n, C.byref(gu)), "svo_ba_solve_forms")
        return list(out), gu.value

    def set_yield_iterations(self, n):
        """LM iterations a wide device-resident solve of this adjuster runs per launch before it steps aside and is launched again
        (0: never, -1: SVO_BA_YIELD_ITERS, else never)."""
        self.ctx._chk(self.L.svo_ba_set_yield_iterations(self.h, int(n)), "svo_ba_set_yield_iterations")

    def solve_resumes(self):
        """Continuation launches of this adjuster's finished wide solves that stepped aside (set_yield_iterations)."""
        n = self.L.svo_ba_wave_chunks_limit() + 2
        out = (C.c_long * n)()
        self.ctx._chk(self.L.svo_ba_solve_forms(self.h, out, n, None), "svo_ba_solve_forms")
        return out[n - 1]

    @staticmethod
    def solve_problems(bas):
        """solve_problem for the loaded problems of several adjusters of one context at once: the admitted wide solves share ONE launch
        (as the lanes of a pipeline group do).  Returns (solves in the shared launch, [BASummary])."""
        n = len(bas)
        hs = (C.c_void_p * n)(*[b.h for b in bas])
        sums = (BASummary * n)()
        rc = bas[0].L.svo_ba_solve_problems(hs, n, sums)
        if rc < 0:
            bas[0].ctx._chk(rc, "svo_ba_solve_problems")
        return rc, list(sums)

    def last_stats(self):
        st = LmStats()
        self.ctx._chk(self.L.svo_ba_last_stats(self.h, C.byref(st)), "svo_ba_last_stats")
        return st

    def read_problem(self):
        K, N = self._shape
        poses = np.empty((K, 7))
        pts = np.empty((N, 3))
        self.ctx._chk(self.L.svo_ba_read_problem(self.h, _p(poses), _p(pts)), "svo_ba_read_problem")
        return poses, pts

    def add_keyframe(self, pose7, tracked_ids, tracked_xy, new_xy, new_xyz):
        pose7 = _f64(pose7)
        tid = np.ascontiguousarray(tracked_ids, np.int64)
        txy, nxy, nxyz = _f32(tracked_xy), _f32(new_xy), _f32(new_xyz)
        nn = nxy.shape[0] if nxy.ndim == 2 else 0
        ids = np.empty(max(nn, 1), np.int64)
        m = C.c_int(0)
        self.ctx._chk(self.L.svo_ba_add_keyframe(self.h, _p(pose7), _p(tid), _p(txy), tid.shape[0], _p(nxy),
                                                 _p(nxyz), nn, _p(ids), C.byref(m)), "svo_ba_add_keyframe")
        return ids[:m.value].copy()

    def solve(self):
        s = BASummary()
        self.ctx._chk(self.L.svo_ba_solve(self.h, C.byref(s)), "svo_ba_solve")
        return s

    def get_pose(self, k=-1):
        p = np.empty(7)
        self.ctx._chk(self.L.svo_ba_get_pose(self.h, k, _p(p)), "svo_ba_get_pose")
        return p

    def window_count(self):
        return self.L.svo_ba_window_count(self.h)

    def get_points(self, ids):
        ids = np.ascontiguousarray(ids, np.int64)
        out = np.empty((ids.shape[0], 3), np.float32)
        self.ctx._chk(self.L.svo_ba_get_points(self.h, _p(ids), ids.shape[0], _p(out)), "svo_ba_get_points")
        return out


def rccl_unique_id():
    """128-byte ncclUniqueId (bytes) from the librccl the library binds; distribute it to every rank out of band."""
    buf = C.create_string_buffer(128)
    if lib().svo_rccl_unique_id(buf) != 0:
        raise SvoError("svo_rccl_unique_id failed (librccl not available?)")
    return buf.raw


def rccl_comm_create(n_ranks, rank, id128, device):
    comm = C.c_void_p()
    rc = lib().svo_rccl_comm_create(C.byref(comm), n_ranks, rank, C.c_char_p(id128), device)
    if rc != 0:
        raise SvoError(f"svo_rccl_comm_create failed ({rc})")
    return comm.value


def rccl_comm_destroy(comm):
    lib().svo_rccl_comm_destroy.argtypes = [C.c_void_p]
    lib().svo_rccl_comm_destroy(comm)


def ba_default_options():
    o = BAOptions()
    lib().svo_ba_default_options(C.byref(o))
    return o


def pipeline_default_params():
    p = PipelineParams()
    lib().svo_pipeline_default_params(C.byref(p))
    return p


class _KeyframeCloudMethods:
    """What Pipeline and PipelineGroup both offer on their keyframe clouds.  `_ENTRY` is the C entry prefix, "svo_pipeline" or
    "svo_pipeline_group": every method below calls (and, on failure, names) the entry `_ENTRY + "_" + <its own name>`."""

    def _kfc(self, name, *args):
        name = self._ENTRY + "_" + name
        self.ctx._chk(getattr(self.L, name)(self.h, *args), name)

    def set_keyframe_speckle_filter(self, max_size=None, max_diff16=0):
        """svo_pipeline[_group]_set_keyframe_speckle_filter: the keyframe maps are speckle-filtered before the clouds are formed (clouds
        must be on; group-wide in a group); max_size None: off."""
        self._kfc("set_keyframe_speckle_filter", _ref(None if max_size is None else SpeckleParams(int(max_size), int(max_diff16))))

    def set_keyframe_lr_check(self, max_diff16=None):
        """svo_pipeline[_group]_set_keyframe_lr_check: the keyframe maps pass the left-right check before the speckle filter and the clouds
        (clouds must be on; group-wide in a group); max_diff16 None: off."""
        self._kfc("set_keyframe_lr_check", _ref(None if max_diff16 is None else LrCheckParams(int(max_diff16))))

    def set_keyframe_sgm(self, p1=None, p2=None, on=True):
        """svo_pipeline[_group]_set_keyframe_sgm: the keyframe maps come from semi-global matching instead of block matching (clouds must
        be on; group-wide in a group); p1 / p2 None: the defaults 2 * 21^2 / 8 * 21^2; on=False: back to block matching."""
        self._kfc("set_keyframe_sgm", _ref(_sgm_params(p1, p2) if on else None))

    def keyframe_clouds(self):
        """The keyframes of the last process call: [{frame, lane, n_total, n_stored, dev, points (CLOUD_POINT_DTYPE array)}], in frame
        order; of a group: over the lanes that have clouds on, ordered by lane, then frame."""
        return _keyframe_clouds(self.ctx, self.L, self.h, getattr(self.L, self._ENTRY + "_keyframe_clouds"),
                                getattr(self.L, self._ENTRY + "_copy_keyframe_cloud"))

    def keyframe_disparity(self, i):
        """svo_pipeline[_group]_keyframe_disparity: the device pointer (an int) of the tight CV_16S map of entry i of keyframe_clouds(), as
        its cloud was formed from it; valid until the next process call."""
        return _keyframe_disparity(self.ctx, self.h, getattr(self.L, self._ENTRY + "_keyframe_disparity"), i)

    def copy_keyframe_disparity(self, i):
        """svo_pipeline[_group]_copy_keyframe_disparity: entry i's map as a (height, width) int16 numpy array (synchronous)."""
        return _keyframe_disparity_host(self.ctx, self.h, getattr(self.L, self._ENTRY + "_copy_keyframe_disparity"), i, self.prm.width, self.prm.height)


class Pipeline(_KeyframeCloudMethods):
    """svo_pipeline wrapper: ImageProcessor::process + BundleAdjuster::bundle_adjust per frame."""

    _ENTRY = "svo_pipeline"

    def __init__(self, ctx, params):
        self.ctx, self.L, self.prm = ctx, ctx.L, params
        self.h = C.c_void_p()
        ctx._chk(self.L.svo_pipeline_create(ctx.h, C.byref(self.h), C.byref(params)), "svo_pipeline_create")
        self.L.svo_pipeline_destroy.argtypes = [C.c_void_p]

    def close(self):
        if self.h:
            self.L.svo_pipeline_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        self.ctx._chk(self.L.svo_pipeline_reset(self.h), "svo_pipeline_reset")

    def set_rectification(self, left=None, right=None):
        """svo_pipeline_set_rectification: RectifyEye per eye (left/right are raw images from then on); None, None: off."""
        self.L.svo_pipeline_set_rectification.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        self.ctx._chk(self.L.svo_pipeline_set_rectification(self.h, _ref(left), _ref(right)), "svo_pipeline_set_rectification")

    def set_keyframe_clouds(self, params=None, max_keyframes_per_call=0):
        """svo_pipeline_set_keyframe_clouds: params a CloudParams (max_points <= 0: width*height), or True for the defaults; None: off."""
        if params is True:
            params = cloud_default_params(self.prm.width, self.prm.height)
        self.ctx._chk(self.L.svo_pipeline_set_keyframe_clouds(self.h, _ref(params), max_keyframes_per_call),
                      "svo_pipeline_set_keyframe_clouds")

    def process_batch(self, left, right):
        """left/right: (B, H, W) uint8 host arrays."""
        left, right = _u8(left), _u8(right)
        b = left.shape[0]
        res = (FrameResult * b)()
        self.ctx._chk(self.L.svo_pipeline_process_batch(self.h, _p(left), _p(right), b, res), "svo_pipeline_process_batch")
        return list(res)

    def process_batch_dev(self, left_ptr, right_ptr, batch):
        """left_ptr/right_ptr: raw device pointers (ints) to (B, H, W) uint8 images resident in HBM."""
        res = (FrameResult * batch)()
        self.ctx._chk(self.L.svo_pipeline_process_batch_dev(self.h, C.c_void_p(left_ptr), C.c_void_p(right_ptr), batch, res),
                      "svo_pipeline_process_batch_dev")
        return list(res)

    def draw_track(self, keyframe_gray):
        """RGB drawing of the tracker state over the (host) keyframe image: FeatureTracker::draw_track + get_drawing."""
        g = np.ascontiguousarray(keyframe_gray, np.uint8)
        out = np.empty(g.shape + (3,), np.uint8)
        self.ctx._chk(self.L.svo_pipeline_draw_track(self.h, _p(g), g.shape[1], _p(out)), "svo_pipeline_draw_track")
        return out

    def tracked(self, capacity=8192):
        ids = np.empty(capacity, np.int64)
        xy = np.empty((capacity, 2), np.float32)
        n = C.c_int(0)
        self.ctx._chk(self.L.svo_pipeline_get_tracked(self.h, _p(ids), _p(xy), capacity, C.byref(n)), "svo_pipeline_get_tracked")
        return ids[:n.value].copy(), xy[:n.value].copy()


class PipelineGroup(_KeyframeCloudMethods):
    """svo_pipeline_group wrapper: n_lanes independent stereo streams behind one caller thread (stream-batched launches)."""

    _ENTRY = "svo_pipeline_group"
    STAGES = ("track", "pnp_ransac", "host_thread_busy_us_of_call_us", "dedup_stereo_triangulate", "bundle_adjust", "corners_pyramids")

    def __init__(self, ctx, params, n_lanes):
        self.ctx, self.L, self.prm, self.n_lanes = ctx, ctx.L, params, n_lanes
        self.h = C.c_void_p()
        self.L.svo_pipeline_group_destroy.argtypes = [C.c_void_p]
        self.L.svo_pipeline_group_destroy.restype = None
        self.L.svo_pipeline_group_process_batch_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        ctx._chk(self.L.svo_pipeline_group_create(ctx.h, C.byref(self.h), C.byref(params), n_lanes), "svo_pipeline_group_create")

    def close(self):
        if self.h:
            self.L.svo_pipeline_group_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        self.ctx._chk(self.L.svo_pipeline_group_reset(self.h), "svo_pipeline_group_reset")

    def set_rectification(self, lane, left=None, right=None):
        """svo_pipeline_group_set_rectification: lane -1 = every lane; None, None turns the lane's rectification off."""
        self.L.svo_pipeline_group_set_rectification.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        self.ctx._chk(self.L.svo_pipeline_group_set_rectification(self.h, lane, _ref(left), _ref(right)), "svo_pipeline_group_set_rectification")

    def set_keyframe_clouds(self, lane=-1, params=None, max_keyframes_per_call=0):
        """svo_pipeline_group_set_keyframe_clouds: lane -1 = every lane; params a CloudParams, True for the defaults, None: off."""
        if params is True:
            params = cloud_default_params(self.prm.width, self.prm.height)
        self.ctx._chk(self.L.svo_pipeline_group_set_keyframe_clouds(self.h, lane, _ref(params), max_keyframes_per_call),
                      "svo_pipeline_group_set_keyframe_clouds")

    def process_batch_dev(self, left_ptr, right_ptr, lane_stride, batch):
        """left_ptr/right_ptr: raw device pointers to (n_lanes, B, H, W) uint8 images (lane_stride bytes between lanes).
        Returns a list of n_lanes lists of FrameResult."""
        res = (FrameResult * (self.n_lanes * batch))()
        self.ctx._chk(self.L.svo_pipeline_group_process_batch_dev(self.h, C.c_void_p(left_ptr), C.c_void_p(right_ptr), C.c_size_t(lane_stride),
                                                                  batch, res), "svo_pipeline_group_process_batch_dev")
        self.last_raw = bytes(res)  # every lane's results as the library wrote them (it zeroes the records first): bench.py's bit-for-bit checks
        return [list(res[l * batch:(l + 1) * batch]) for l in range(self.n_lanes)]

    def staging(self, slot):
        """The slot's pinned staging buffers as numpy views (n_lanes, max_batch, H, W): the caller fills them in place."""
        lp, rp, stride = C.POINTER(C.c_uint8)(), C.POINTER(C.c_uint8)(), C.c_size_t(0)
        self.L.svo_pipeline_group_staging.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        self.ctx._chk(self.L.svo_pipeline_group_staging(self.h, slot, C.byref(lp), C.byref(rp), C.byref(stride)), "svo_pipeline_group_staging")
        h, w = self.prm.height, self.prm.width
        mb = stride.value // (h * w)
        shape = (self.n_lanes, mb, h, w)
        n = self.n_lanes * mb * h * w
        return (np.ctypeslib.as_array(lp, shape=(n,)).reshape(shape), np.ctypeslib.as_array(rp, shape=(n,)).reshape(shape))

    def upload(self, slot, batch):
        self.ctx._chk(self.L.svo_pipeline_group_upload(self.h, slot, batch), "svo_pipeline_group_upload")

    def process_uploaded(self, slot, batch):
        res = (FrameResult * (self.n_lanes * batch))()
        self.L.svo_pipeline_group_process_uploaded.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        self.ctx._chk(self.L.svo_pipeline_group_process_uploaded(self.h, slot, res), "svo_pipeline_group_process_uploaded")
        self.last_raw = bytes(res)
        return [list(res[l * batch:(l + 1) * batch]) for l in range(self.n_lanes)]

    def process_batch(self, left, right):
        """left/right: (n_lanes, B, H, W) uint8 HOST arrays (the convenience entry: copy into slot 0, upload, process)."""
        left, right = _u8(left), _u8(right)
        batch = left.shape[1]
        res = (FrameResult * (self.n_lanes * batch))()
        self.L.svo_pipeline_group_process_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        self.ctx._chk(self.L.svo_pipeline_group_process_batch(self.h, _p(left), _p(right), C.c_size_t(batch * left.shape[2] * left.shape[3]), batch, res),
                      "svo_pipeline_group_process_batch")
        self.last_raw = bytes(res)
        return [list(res[l * batch:(l + 1) * batch]) for l in range(self.n_lanes)]

    def get_tracked(self, lane, capacity=8192):
        ids = np.empty(capacity, np.int64)
        xy = np.empty((capacity, 2), np.float32)
        n = C.c_int(0)
        self.ctx._chk(self.L.svo_pipeline_group_get_tracked(self.h, lane, _p(ids), _p(xy), capacity, C.byref(n)), "svo_pipeline_group_get_tracked")
        return ids[:n.value].copy(), xy[:n.value].copy()

    def solve_work(self, reset=False):
        """Algorithmic [f64 flops, bytes, solves, LM iterations] of the bundle adjustments finished since the last reset."""
        out = (C.c_double * 4)()
        self.ctx._chk(self.L.svo_pipeline_group_solve_work(self.h, out, int(reset)), "svo_pipeline_group_solve_work")
        return list(out)

    def solve_forms(self):
        """([compact solves, wide solves at k = 1, 2, ... chunks per wavefront], solves that gave up and were run again), summed over the
        lanes' adjusters since the group was created."""
        n = self.L.svo_ba_wave_chunks_limit() + 1
        out, gu = (C.c_long * n)(), C.c_long(0)
        self.ctx._chk(self.L.svo_pipeline_group_solve_forms(self.h, out, n, C.byref(gu)), "svo_pipeline_group_solve_forms")
        return list(out), gu.value

    def set_solve_yield(self, n):
        """LM iterations a lane's wide window solve runs per launch before it steps aside and rides the group's next wide launch (0: never)."""
        self.ctx._chk(self.L.svo_pipeline_group_set_solve_yield(self.h, int(n)), "svo_pipeline_group_set_solve_yield")

    def solve_resumes(self):
        """Continuation launches of the lanes' finished wide solves that stepped aside, since the group was created."""
        n = self.L.svo_ba_wave_chunks_limit() + 2
        out = (C.c_long * n)()
        self.ctx._chk(self.L.svo_pipeline_group_solve_forms(self.h, out, n, None), "svo_pipeline_group_solve_forms")
        return out[n - 1]

    def last_stats(self):
        """{stage: (launches, lane-stages carried)} of the last process_batch_dev call; "host_thread_busy_us_of_call_us": (microseconds of the
        driving thread's loop passes that did something, microseconds of the call's main loop)."""
        a, b = (C.c_long * 6)(), (C.c_long * 6)()
        self.ctx._chk(self.L.svo_pipeline_group_last_stats(self.h, a, b), "svo_pipeline_group_last_stats")
        return {s: (a[i], b[i]) for i, s in enumerate(self.STAGES) if s != "unused"}


class RunStats(C.Structure):
    _fields_ = [("frames", C.c_int), ("keyframes", C.c_int), ("ate_rmse", C.c_double), ("seconds", C.c_double)]


def image_read_gray(path, max_pixels=1 << 24):
    buf = np.empty(max_pixels, np.uint8)
    w, h = C.c_int(0), C.c_int(0)
    rc = lib().svo_image_read_gray(path.encode(), _p(buf), C.c_size_t(max_pixels), C.byref(w), C.byref(h))
    if rc:
        raise SvoError(f"svo_image_read_gray({path}) rc={rc}")
    return buf[:w.value * h.value].reshape(h.value, w.value).copy()


def kitti_read_poses(path, max_frames=100000):
    rt = np.empty((max_frames, 12))
    n = C.c_int(0)
    rc = lib().svo_kitti_read_poses(path.encode(), _p(rt), max_frames, C.byref(n))
    if rc:
        raise SvoError(f"svo_kitti_read_poses({path}) rc={rc}")
    return rt[:n.value].reshape(-1, 3, 4).copy()


def ate_rmse(est_xyz, gt_xyz, with_scale=False):
    est_xyz, gt_xyz = _f64(est_xyz), _f64(gt_xyz)
    out = C.c_double(0)
    rc = lib().svo_ate_rmse(_p(est_xyz), _p(gt_xyz), est_xyz.shape[0], int(with_scale), C.byref(out))
    if rc:
        raise SvoError(f"svo_ate_rmse rc={rc}")
    return out.value


def kitti_run(ctx, params, data_path, sequence, max_frames):
    """Non-ROS driver over a KITTI-layout directory (data_path must end with '/')."""
    traj = np.zeros((max_frames, 12))
    st = RunStats()
    ctx._chk(lib().svo_kitti_run(ctx.h, C.byref(params), data_path.encode(), sequence, max_frames, _p(traj), C.byref(st)),
             "svo_kitti_run")
    return traj[:st.frames].reshape(-1, 3, 4).copy(), st


def cholesky_solve(A, b):
    """svo_cholesky_solve on copies: returns x with (L L^T) x = b, or raises SvoError when A is not SPD."""
    A = np.array(A, np.float64, order="C")
    b = np.array(b, np.float64)
    rc = lib().svo_cholesky_solve(_p(A), _p(b), b.shape[0])
    if rc != 0:
        raise SvoError(f"svo_cholesky_solve rc={rc}")
    return b


def draw_track(gray, from_xy, to_xy):
    """svo_draw_track: gray (H, W) uint8 -> RGB (H, W, 3) with a green arrow per (from, to) pair."""
    g = np.ascontiguousarray(gray, np.uint8)
    a = np.ascontiguousarray(from_xy, np.float32).reshape(-1, 2)
    b = np.ascontiguousarray(to_xy, np.float32).reshape(-1, 2)
    out = np.empty(g.shape + (3,), np.uint8)
    rc = lib().svo_draw_track(_p(g), g.shape[1], g.shape[0], g.shape[1], _p(a), _p(b), a.shape[0], _p(out))
    if rc:
        raise SvoError(f"svo_draw_track rc={rc}")
    return out
