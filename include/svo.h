/*
 * svo.h — C-ABI drop-in boundary of the MI355X-native stereo-VO hot path.
 *
 * Every entry point replaces one call the reference's ImageProcessor /
 * FeatureTracker / BundleAdjuster make into OpenCV / Ceres (reference
 * file:line is cited on each declaration; paths are relative to the
 * reference repository root).  Plain pointers and sizes only: no C++ types,
 * no torch types.  All functions return 0 (SVO_OK) on success and a negative
 * svo_status otherwise; nothing ever throws across this boundary.  The
 * reference's own error convention is "void + early return" (SURVEY §8b), so a
 * C++ adapter maps a non-zero status to "skip this frame".
 *
 * Memory spaces: functions without a suffix take caller-owned HOST pointers
 * (the boundary the reference classes would bind); functions ending in `_dev`
 * take DEVICE pointers (HBM resident; what the in-library pipeline and
 * bench.py use) and are asynchronous on svo_stream(ctx) unless stated.
 *
 * Threading: one caller thread per context (the reference's vo_node is
 * single-threaded, src/vo_node.cpp:139-227).
 */
#ifndef SVO_H_
#define SVO_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum svo_status {
  SVO_OK = 0,
  SVO_ERR_INVALID = -1,   /* bad argument / shape */
  SVO_ERR_HIP = -2,       /* a HIP runtime call failed (see svo_last_error) */
  SVO_ERR_CAPACITY = -3,  /* a workspace bound given at svo_create was exceeded */
  SVO_ERR_NO_DEVICE = -4, /* no gfx950 device visible */
  SVO_ERR_NUMERIC = -5    /* singular system / non-finite value */
} svo_status;

/* Mirrors struct CameraInfo, src/camera_info.hpp:4-18 (same field order, so a
 * reference CameraInfo can be reinterpret_cast).  focal/cx/cy/baseline describe the ideal, row-aligned pinhole pair
 * every stage works in.  k1..p2 (src/camera_info.hpp:10-14) are not read by svo_pipeline_create, svo_ba_create or any
 * stage: they are honoured where the caller asks for it, through svo_rectify_eye_from_camera_info and the
 * svo_*_set_rectification entries below (the reference itself passes zeros, src/vo_node.cpp:110). */
typedef struct svo_camera_info {
  double focal, cx, cy;
  double k1, k2, p1, p2;
  double baseline;
} svo_camera_info;

typedef struct svo_ctx svo_ctx;

/* Limits fixed at context creation (workspace is allocated once; no
 * allocation happens on the hot path). */
typedef struct svo_limits {
  int max_width, max_height; /* largest image */
  int max_batch;             /* frames per batched front-end call */
  int max_corners;           /* corners returned per image (ref: 300, src/image_processor.cpp:22) */
  int max_candidates;        /* NMS survivors per image before min-distance selection */
  int max_features;          /* tracked features per frame (ref: 400, src/bundle_adjuster.hpp:75) */
} svo_limits;

/* Environment knobs read at creation (deployment tuning, no effect on results):
 *   SVO_BA_CU_SHARE=n   when several stereo streams share one GPU: window-sized bundle adjusters (svo_ba_create with
 *                       max_observations <= 100000) launch on their own n compute units of every 32 and the
 *                       context's stream on the remaining ones (HIP CU-masked streams).  n = 8 is one shader engine
 *                       per XCD on MI355X; measured +12 % frames/s at 8 streams per GPU, -2 % with a single stream.
 *                       Unset / 0: both use the whole GPU. */
int svo_create(svo_ctx** out, int device, const svo_limits* limits);
void svo_destroy(svo_ctx* ctx);
const char* svo_last_error(const svo_ctx* ctx);
/* hipStream_t the context launches on (as void*). */
void* svo_stream(svo_ctx* ctx);
int svo_sync(svo_ctx* ctx);
/* library build tag; "gfx950" must appear in it. */
const char* svo_version(void);

/* The reference's first-party literals as compiled into the kernels and the host chain (csrc/ref_constants.h), for
 * audit: tests check them against values extracted from the reference's source text (tests/golden/constants_golden.json).
 * All doubles; names follow that fixture.  Reference lines: src/image_processor.cpp:22,23,63,80,174,176,194,
 * src/feature_tracker.cpp:24-26,47,53,81, src/vo_node.cpp:33-36, src/bundle_adjuster.hpp:75, src/bundle_adjuster.cpp:11-12. */
typedef struct svo_reference_constants_t {
  double gftt_max_corners, gftt_quality, min_detected, keyframe_percent_lost;
  double pnp_iterations, pnp_reproj_error, pnp_confidence;
  double stereo_num_disparities, stereo_block_size, stereo_disparity_scale, triangulate_min_disparity_exclusive;
  double lk_win_w, lk_win_h, lk_max_level, lk_max_iterations, lk_epsilon, lk_min_eig_threshold;
  double fb_max_distance, max_parallax, draw_thickness;
  double parallax_thresh, min_feature_distance, sliding_window_size, max_features;
  double ba_max_solver_time_s, ba_num_threads;
} svo_reference_constants_t;
int svo_reference_constants(svo_reference_constants_t* out);

/* Measurement aid (not a reference interface): time every launch of ONE named kernel with HIP events
 * recorded on the context stream.  kernel: "corner_response", "corner_nms", "corner_select", "pyr_down",
 * "lk_fb", "stereo_at", "triangulate", "pnp_hypotheses", "pnp_refine", "ba_linearize", "ba_backsub", "ba_step",
 * "rectify_remap", "stereo_bm" (the three launches of svo_stereo_bm as one bracket), "stereo_dense_batch",
 * "cloud" (the count, scan and write launches of one svo_disparity_cloud_batch_dev as one bracket),
 * "speckle" (the launches of one speckle filter call as one bracket), "lr_check" (one left-right check call),
 * "stereo_sgm" (the launches of one semi-global matching call as one bracket), "voxel_insert" (one svo_voxel_map_insert_dev),
 * "voxel_extract" (one svo_voxel_map_extract_dev: the counts' memset and the launch), "voxel_carve" (one
 * svo_voxel_map_carve_dev: the counts' memset and the launch), "voxel_copy" (one svo_voxel_map_copy_live_dev), "voxel_render" (one
 * svo_voxel_map_render_dev: the two memsets and both launches), "voxel_remove" (one svo_voxel_map_remove_dev: the counts' memset and
 * the launch), "voxel_move" (one svo_voxel_map_move_dev: the counts' memset, the removal and the insert; the launches inside it
 * are not counted as "voxel_remove" or "voxel_insert"), "voxel_grid" (one svo_voxel_map_grid_dev: the memsets of the workspace
 * and the counts and both launches), "grid_clearance" (one svo_grid_clearance_dev: the counts' memset and both launches),
 * "grid_route" (one svo_grid_route_dev: its memsets and every launch), "grid_frontier" (one svo_grid_frontiers_dev: the counts'
 * memset and every launch), "grid_view" (one svo_grid_view_dev: its two memsets and both launches), "grid_surface" (one svo_grid_surface_dev: the
 * counts' memset and the launch), "grid_waypoints" (one svo_grid_waypoints_dev: the counts' memset and the launch),
 * "voxel_align" (one svo_voxel_map_align_sums_dev: the sums' memset and the launch; svo_voxel_map_align is one bracket per
 * iteration), "voxel_normals" (one svo_voxel_map_normals_dev), "voxel_align_plane" (one svo_voxel_map_align_plane_sums_dev),
 * "voxel_occupancy" (one svo_voxel_map_occupancy_dev: its two memsets and the launch), "voxel_locate" (one
 * svo_voxel_map_locate_scores_dev: its memsets, the score launches and the best launch; the occupancy launch and the
 * refinements inside svo_voxel_map_locate count under their own tags), "voxel_coarse" (one svo_voxel_occupancy_coarse_dev: its memset
 * and the launch), "voxel_rays" (one svo_voxel_occupancy_rays_dev or _raycast_dev: the counts' memset and the launch),
 * "voxel_distance" (one svo_voxel_occupancy_distance_dev: the counts' memset and its three launches), "voxel_distance_query" (one
 * svo_voxel_distance_query_dev: the counts' memset and the launch), "voxel_route" (one svo_voxel_occupancy_route_dev: its memsets and
 * every launch); NULL/"" disables.  svo_profile_read synchronises the stream and returns the summed duration and the
 * launch count since the last svo_profile_select. */
int svo_profile_select(svo_ctx* ctx, const char* kernel);
/* Measurement aid: the card's own ceilings for the roofline objects (SURVEY 8d asks for a measured FP64 figure).
 * what: "f64_fma" (vector FMA), "f64_muladd" (separate multiply + add: what the parity-exact kernels issue),
 * "f64_mfma" (v_mfma_f64_16x16x4_f64), "hbm_copy" (512 MiB device copy).  *value: flop/s or bytes/s (read + write). */
int svo_measure_peak(svo_ctx* ctx, const char* what, double* value);
int svo_profile_read(svo_ctx* ctx, double* total_ms, int* launches);

/* ------------------------------------------------------------- rectification --
 * Raw (distorted, not row-aligned) stereo pairs -> the ideal pinhole pair the pipeline assumes, on the device.  The
 * reference has no counterpart: it carries k1, k2, p1, p2 in CameraInfo (src/camera_info.hpp:10-14), never reads them and
 * is fed rectified images (src/vo_node.cpp:110).  One svo_rectify_eye describes one RAW camera; the rectified camera is
 * the svo_camera_info (focal, cx, cy) of the call, the same for both eyes.  Raw and rectified images have the same size.
 *
 * The warp is a precomputed table (one 4-byte record per destination pixel) applied by rectify_remap_kernel:
 *   map   all f64, every operation rounded separately, only + - x / and rint (host/rectify.cpp states the order): the
 *         construction of OpenCV's initUndistortRectifyMap followed by its 1/32-pixel fixed-point maps.  Record of pixel
 *         (u, v): int16 dx = qx - 32 u, int16 dy = qy - 32 v with (qx, qy) the source position in 1/32 pixels;
 *         (-32768, -32768) = no source (behind the camera, non-finite, or all four taps outside the raw image);
 *   remap bilinear in exact integers: weights (32-ax)(32-ay), ax(32-ay), (32-ax)ay, ax ay (sum 1024), output
 *         (sum w p + 512) >> 10, a tap outside the raw image contributes 0, a pixel without source is 0.  The intent: the
 *         integers of OpenCV's fixed-point INTER_LINEAR remap with a constant-0 border (its 15-bit table is these weights
 *         times 32); what is pinned by the tests is the arithmetic declared here. */
typedef struct svo_rectify_eye {
  double fx, fy, cx, cy;   /* camera matrix of the RAW image */
  double k1, k2, p1, p2;   /* Brown-Conrady coefficients, in CameraInfo's order (src/camera_info.hpp:10-14) */
  double R[9];             /* row-major rotation raw camera -> rectified camera (identity: undistortion only) */
} svo_rectify_eye;
/* The monocular case of a CameraInfo (src/camera_info.hpp:4-18): fx = fy = focal, the same centre, k1..p2 copied, R = I. */
int svo_rectify_eye_from_camera_info(const svo_camera_info* cam, svo_rectify_eye* eye);
/* The table itself (src/camera_info.hpp:10-14 are its coefficients).  Host-only, needs no GPU.  dxdy: width x height x 2
 * int16, row-major, (dx, dy) per pixel.  A source inside the raw image whose displacement does not fit an int16 (beyond
 * +-32767 / 32 px) is never clipped: SVO_ERR_INVALID, and svo_last_error(NULL) names it (per thread). */
int svo_rectify_build_map(const svo_rectify_eye* eye, const svo_camera_info* cam, int width, int height, int16_t* dxdy);
/* One image, HOST pointers (coefficients: src/camera_info.hpp:10-14): out (tight rows) = raw warped by the table of
 * (eye, cam).  Stand-alone use; also how a caller gets the rectified keyframe image svo_pipeline_draw_track wants. */
int svo_rectify_remap(svo_ctx* ctx, const uint8_t* raw, int width, int height, int row_stride, const svo_rectify_eye* eye,
                      const svo_camera_info* cam, uint8_t* out);
/* `batch` images of one camera (src/camera_info.hpp:10-14), DEVICE pointers, one launch: raw images image_stride bytes
 * apart with rows row_stride bytes apart; out: tight rows, images width*height bytes apart.  The table is built and
 * uploaded by the call (synchronous with respect to the host, asynchronous launch on svo_stream(ctx)). */
int svo_rectify_remap_batch_dev(svo_ctx* ctx, const uint8_t* raw, int batch, int width, int height, int row_stride,
                                size_t image_stride, const svo_rectify_eye* eye, const svo_camera_info* cam, uint8_t* out);

/* ------------------------------------------------------------------ a11 --
 * Batched ReprojectionFactor::Evaluate (src/reprojection_factor.cpp:10-88).
 * pose7 = [qw qx qy qz tx ty tz] (src/bundle_adjuster.hpp:50), n of them;
 * point3, obs2 likewise.  r2: n x 2.  jpose14: n x (2x7 row-major) or NULL;
 * jpoint6: n x (2x3 row-major) or NULL (Ceres' null conventions,
 * src/reprojection_factor.cpp:58-59,77).  Entries 5 and 11 of each 2x7 are 0
 * (src/reprojection_factor.cpp:61). */
int svo_reproj_eval(svo_ctx* ctx, int n, const double* pose7, const double* point3,
                    const double* obs2, double focal, double cx, double cy,
                    double* r2, double* jpose14, double* jpoint6);
int svo_reproj_eval_dev(svo_ctx* ctx, int n, const double* pose7, const double* point3,
                        const double* obs2, double focal, double cx, double cy,
                        double* r2, double* jpose14, double* jpoint6);

/* ------------------------------------------------------------------- a1 --
 * cv::goodFeaturesToTrack(img, out, max_corners, quality, min_distance)
 * with defaults blockSize=3, useHarris=false, no mask
 * (call site src/image_processor.cpp:22; semantics SURVEY Appendix A.1).
 * xy: max_corners x 2 floats (integer-valued pixel coords, strongest first);
 * *n receives the count.  Batched form: images are `image_stride` bytes
 * apart, rows `row_stride` bytes apart; xy is batch x max_corners x 2,
 * n is batch ints. */
int svo_corner_detect(svo_ctx* ctx, const uint8_t* img, int width, int height, int row_stride,
                      int max_corners, double quality, double min_distance,
                      float* xy, int* n);
int svo_corner_detect_batch_dev(svo_ctx* ctx, const uint8_t* imgs, int batch, int width, int height,
                                int row_stride, size_t image_stride, int max_corners,
                                double quality, double min_distance, float* xy, int* n);
/* Debug/parity taps of the same path: the min-eigenvalue map (float, width*height)
 * produced by the response kernel. Host pointers. */
int svo_corner_response(svo_ctx* ctx, const uint8_t* img, int width, int height, int row_stride,
                        float* eig);

/* ------------------------------------------------------------------- a7 --
 * cv::StereoBM::create(num_disp, block)->compute(L,R) + convertTo(CV_32F,1/16)
 * (src/image_processor.cpp:173-176; defaults XSOBEL cap 31,
 * minDisparity 0, textureThreshold 10, uniquenessRatio 15).
 * Dense form writes the CV_16S map (4 fractional bits, FILTERED = -16).
 * Sparse form evaluates exactly the same function only at (int)y,(int)x of
 * each point (what src/image_processor.cpp:193 samples) and returns the
 * float disparity (-1.0 = filtered). */
int svo_stereo_bm(svo_ctx* ctx, const uint8_t* left, const uint8_t* right, int width, int height,
                  int row_stride, int num_disparities, int block_size, int16_t* disp16);
int svo_stereo_disparity_at(svo_ctx* ctx, const uint8_t* left, const uint8_t* right, int width,
                            int height, int row_stride, int num_disparities, int block_size,
                            const float* xy, int n, float* disp);
int svo_stereo_disparity_at_dev(svo_ctx* ctx, const uint8_t* left, const uint8_t* right, int width,
                                int height, int row_stride, int num_disparities, int block_size,
                                const float* xy, const int* n_dev, int n_max, float* disp);

/* ------------------------------------------------------- dense depth clouds --
 * The dense form of ImageProcessor::triangulate_stereo (src/image_processor.cpp:173-207): the whole StereoBM map instead of
 * its samples at the feature pixels, and one 3-D point per kept pixel instead of one per feature.
 *
 * svo_stereo_bm_batch_dev (src/image_processor.cpp:173-207, the compute() of :174-175): `batch` pairs in ONE launch, DEVICE
 * pointers, asynchronous on svo_stream(ctx).  Pair b's images start b * image_stride bytes after left / right, rows row_stride
 * bytes apart; disp16: batch tight CV_16S maps (width*height each), bit-identical to svo_stereo_bm.  The raw images are read
 * directly (the X-Sobel prefilter is formed in LDS).  Argument limits as svo_stereo_bm; 1 <= batch <= svo_limits.max_batch. */
int svo_stereo_bm_batch_dev(svo_ctx* ctx, const uint8_t* left, const uint8_t* right, int batch, int width, int height,
                            int row_stride, size_t image_stride, int num_disparities, int block_size, int16_t* disp16);
/* Which pixels of a map become points (src/image_processor.cpp:173-207; the test of :194 generalised): pixel (x, y) is kept
 * iff x % step == 0, y % step == 0 and d > max(min_disparity, 0) with d = (float)disp16 * 0.0625f (the convertTo of :176).
 * max_points bounds what is STORED per image, never what is counted. */
typedef struct svo_cloud_params {
  int step;             /* 1 */
  float min_disparity;  /* 0 */
  int max_points;       /* <= 0 in svo_pipeline*_set_keyframe_clouds: width*height */
} svo_cloud_params;
/* Defaults for a width x height map (src/image_processor.cpp:173-207): step 1, min_disparity 0, max_points width*height. */
int svo_cloud_default_params(svo_cloud_params* p, int width, int height);
/* One point of a cloud (src/image_processor.cpp:173-207; arithmetic of :196-204 exactly as svo_triangulate for the feature
 * ((float)x, (float)y) with disparity d).  tag = (y * width + x) | (left[y][x] << 24): pixel index and intensity, hence
 * width*height <= 2^24. */
typedef struct svo_cloud_point {
  float x, y, z;
  uint32_t tag;
} svo_cloud_point;
/* Maps -> compacted point lists in raster order (src/image_processor.cpp:173-207), DEVICE pointers, asynchronous.  disp16:
 * batch tight maps; left: the left images (strides as above; read for the tag only); pose16: batch x 16 f32 row-major
 * camera->world, NULL = identity for every pair; points: batch x params->max_points records; counts: batch x 2 ints,
 * {n_total, n_stored = min(n_total, max_points)} - the first n_stored kept pixels in raster order are stored, records past
 * them are not written.  One count launch, one scan launch, one write launch for the whole batch. */
int svo_disparity_cloud_batch_dev(svo_ctx* ctx, const int16_t* disp16, const uint8_t* left, int batch, int width, int height,
                                  int row_stride, size_t image_stride, const svo_camera_info* cam, const float* pose16,
                                  const svo_cloud_params* params, svo_cloud_point* points, int* counts);
/* One pair, HOST pointers, synchronous (src/image_processor.cpp:173-207 end to end): map + cloud.  pose16: 16 f32 or NULL;
 * points: params->max_points records. */
int svo_stereo_cloud(svo_ctx* ctx, const uint8_t* left, const uint8_t* right, int width, int height, int row_stride,
                     int num_disparities, int block_size, const svo_camera_info* cam, const float* pose16,
                     const svo_cloud_params* params, svo_cloud_point* points, int* n_total, int* n_stored);

/* ---------------------------------------------------------- speckle filter --
 * What cv::filterSpeckles(map, -16, max_size, max_diff16) computes on a CV_16S map (4 fractional bits, FILTERED = -16), on the
 * device, for a batch of maps (no reference counterpart: the reference samples its map at the features and never filters it;
 * a whole-map cloud has to).  The pixels whose value is not FILTERED are the nodes of a graph; two nodes are joined iff they are
 * 4-neighbours and |a - b| <= max_diff16 (in int32: any int16 values are accepted); every connected component with at most
 * max_size nodes is set to FILTERED, nothing else changes.  The result depends on no order.  max_diff16 is in the map's own
 * units of 1/16 pixel.  max_size == 0 is the identity: nothing is launched and n_removed is not written by the _dev entry. */
typedef struct svo_speckle_params {
  int max_size;    /* >= 0, pixels */
  int max_diff16;  /* >= 0, 1/16 pixel */
} svo_speckle_params;
/* The tile of the labelling pass (a removed component that crosses a multiple of these is one that several workgroups agreed on). */
#define SVO_SPECKLE_TILE_W 64
#define SVO_SPECKLE_TILE_H 16
/* Bytes of work space for `batch` maps of width x height: one u32 label and one u32 count per pixel, 8*width*height*batch, no
 * constant on top.  Pure (no device needed); 0 for a shape the filter refuses (width, height, batch < 1, width*height >= 2^31,
 * batch > 65535). */
size_t svo_speckle_workspace_bytes(int width, int height, int batch);
/* `batch` tight maps filtered in place, DEVICE pointers, asynchronous on svo_stream(ctx): one launch sequence (tile labelling,
 * seam merge, count, apply) for the whole batch.  workspace: 4-byte aligned device memory of at least
 * svo_speckle_workspace_bytes(width, height, batch) bytes (nothing behind that is touched; contents before and after are
 * meaningless).  n_removed: `batch` device ints, the number of pixels this call set to FILTERED per map, or NULL. */
int svo_disparity_speckle_filter_batch_dev(svo_ctx* ctx, int16_t* disp16, int batch, int width, int height,
                                           const svo_speckle_params* params, void* workspace, size_t workspace_bytes, int* n_removed);
/* One map, HOST pointers, in place, synchronous; n_removed: host int or NULL. */
int svo_disparity_speckle_filter(svo_ctx* ctx, int16_t* disp16, int width, int height, const svo_speckle_params* params,
                                 int* n_removed);

/* -------------------------------------------------------- left-right check --
 * What disp12MaxDiff of StereoBM switches on (cv::validateDisparity, which StereoBM::compute runs BEFORE filterSpeckles), on the
 * device, for a batch of CV_16S maps (4 fractional bits, FILTERED = -16) and the winner's SAD per pixel (no reference counterpart:
 * the reference leaves disp12MaxDiff off because it samples the map at the features only; a whole-map cloud shows the band of
 * wrong disparities along every depth edge).  Rows are independent; all arithmetic is int32, >> is the arithmetic shift, any
 * int16 values are accepted.  Per row: every x with d = disp16[y][x] != FILTERED votes for the right-view column
 * x2 = x - ((d + 8) >> 4) (a vote outside [0, width) is dropped); a column's winner is the vote with the smallest
 * (cost16[y][x], x) and d2[x2] is the winner's d; a column without a vote is empty.  Then, for every x with d != FILTERED, with
 * xa = x - (d >> 4) and xb = x - ((d + 15) >> 4): a look-up at xq is bad iff 0 <= xq < width, d2[xq] is not empty and
 * |d2[xq] - d| > max_diff16; the pixel becomes FILTERED iff BOTH look-ups are bad.  Nothing else changes.  d2 is formed from the
 * input row, so the result depends on no order.  The check is not idempotent in general (a removed pixel no longer votes).
 * max_diff16 is in the map's own unit of 1/16 pixel: disp12MaxDiff = k pixels is max_diff16 = 16 k. */
typedef struct svo_lr_check_params {
  int max_diff16;  /* >= 0, 1/16 pixel */
} svo_lr_check_params;
/* The widest map the check takes: the row and one 32-bit key per column live in LDS, 6 bytes per column, within the 64 KB a
 * kernel gets without asking.  A wider map is refused with SVO_ERR_INVALID and a message naming this bound. */
#define SVO_LR_CHECK_MAX_WIDTH 10240
/* svo_stereo_bm_batch_dev that also writes cost16[y][x] = the winner's SAD (the minsad of the selection) where the map is not
 * FILTERED and 0xFFFF where it is (a SAD is at most 21*21*62 = 27,342).  The map is bit-identical to svo_stereo_bm_batch_dev's.
 * disp16, cost16: `batch` tight maps each, DEVICE pointers. */
int svo_stereo_bm_cost_batch_dev(svo_ctx* ctx, const uint8_t* left, const uint8_t* right, int batch, int width, int height,
                                 int row_stride, size_t image_stride, int num_disparities, int block_size, int16_t* disp16,
                                 uint16_t* cost16);
/* `batch` tight maps checked in place, DEVICE pointers, asynchronous on svo_stream(ctx): one launch for the whole batch.
 * 1 <= batch <= 65535, 1 <= width <= SVO_LR_CHECK_MAX_WIDTH, height >= 1.  n_removed: `batch` device ints, the number of pixels
 * this call set to FILTERED per map (zeroed on the stream before the launch), or NULL. */
int svo_disparity_lr_check_batch_dev(svo_ctx* ctx, int16_t* disp16, const uint16_t* cost16, int batch, int width, int height,
                                     const svo_lr_check_params* params, int* n_removed);
/* One map, HOST pointers, disp16 in place, synchronous; n_removed: host int or NULL. */
int svo_disparity_lr_check(svo_ctx* ctx, int16_t* disp16, const uint16_t* cost16, int width, int height,
                           const svo_lr_check_params* params, int* n_removed);

/* ------------------------------------------------------ semi-global matching --
 * Four-path cost aggregation over StereoBM's cost volume, then StereoBM's own selection on the aggregated costs, for a batch of
 * pairs on the device (no reference counterpart: the reference samples StereoBM at textured features; a whole-map cloud wants
 * the weakly textured surfaces block matching rejects).  This is the project's own statement; parity with OpenCV's SGBM is NOT
 * claimed.  Inputs as svo_stereo_bm_batch_dev (raw uint8 pairs, num_disparities 16 / 32 / 48 / 64, block_size odd 5..21) plus
 * 0 <= p1 <= p2 <= SVO_SGM_MAX_P2.  All arithmetic is exact integer arithmetic.
 *   1. Cost volume.  Over StereoBM's valid rectangle (x in [ndisp-1+half, W-half), y in [half, H-half), half = block_size / 2)
 *      C(x, y, d) is exactly the windowed SAD of the prefiltered images that StereoBM minimises (same prefilter, same mirrored
 *      rows, same window); the texture sum is StereoBM's.
 *   2. Paths.  Four: left->right, right->left, top->bottom, bottom->top, all inside the valid rectangle.  The first pixel of a
 *      path has L_r(p, d) = C(p, d); after it, with q the previous pixel and m = min_k L_r(q, k),
 *        L_r(p, d) = C(p, d) + min(L_r(q, d), L_r(q, d-1) + p1, L_r(q, d+1) + p1, m + p2) - m,
 *      the d +- 1 terms absent outside [0, ndisp).  Hence L_r <= 27,342 + p2 <= 60,109 (16 bits); S = sum_r L_r <= 240,436.
 *   3. Selection on S: StereoBM's with s := S.  The winner is the minimum, among equal minima the LARGEST d; the pixel is rejected
 *      iff some d more than 1 away from the winner has S <= m + m * 15 / 100 (C division), or iff the texture sum < 10; the
 *      sub-pixel term uses the mirrored ends S[-1] = S[1], S[ndisp] = S[ndisp-2], truncated division and (... + 15) >> 4.
 *      Output: CV_16S, 4 fractional bits, FILTERED = -16; everything outside the rectangle is FILTERED.
 *   4. Cost form.  cost16 = min((S_min + 2) >> 2, 0xFFFE) where the map is not FILTERED, 0xFFFF where it is: what
 *      svo_disparity_lr_check_batch_dev takes.
 *   5. Identity.  With p1 = p2 = 0, map and cost are bit-identical to svo_stereo_bm_cost_batch_dev's (L_r = C, S = 4 C).
 *   6. Defaults.  p1 = 2 block_size^2, p2 = 8 block_size^2: chosen on a synthetic scene, NOT tuned on real imagery. */
typedef struct svo_sgm_params {
  int p1;  /* >= 0: a disparity step of 1 between path neighbours */
  int p2;  /* p1 <= p2 <= SVO_SGM_MAX_P2: any larger step */
} svo_sgm_params;
/* The largest p2: 27,342 + 32,767 = 60,109 keeps a path cost within 16 bits. */
#define SVO_SGM_MAX_P2 32767
/* Keyframe maps of a pipeline / a group are matched this many pairs at a time (svo_pipeline_set_keyframe_sgm): the work space
 * is allocated for this many pairs, whatever max_keyframes_per_call is. */
#define SVO_SGM_KEYFRAME_SUB_BATCH 2
/* p1 = 2 block_size^2, p2 = 8 block_size^2 (block_size odd 5..21, SVO_ERR_INVALID otherwise). */
int svo_sgm_default_params(svo_sgm_params* params, int block_size);
/* Bytes of work space for `batch` pairs: per pixel of the valid rectangle, num_disparities u16 costs and as many u32 sums plus
 * one u16 texture sum, each array rounded up to 256 bytes (about 120 MB per 1241 x 376 pair at 48 disparities); never less than
 * 256 for an accepted shape.  Pure (no device needed); 0 for a refused shape (width or height < 3, width*height > 2^30, batch
 * outside 1..65535, a num_disparities or block_size StereoBM refuses). */
size_t svo_sgm_workspace_bytes(int width, int height, int num_disparities, int block_size, int batch);
/* `batch` pairs, DEVICE pointers, asynchronous on svo_stream(ctx), ordered by launch: fill, cost volume, four path launches (the
 * last one selects).  Images and strides as svo_stereo_bm_batch_dev; 1 <= batch <= svo_limits.max_batch.  workspace: 256-byte
 * aligned device memory of at least svo_sgm_workspace_bytes(...) bytes (nothing behind that is touched; contents before and
 * after are meaningless).  disp16: batch tight maps; cost16: batch tight maps or NULL.  A refused call (null pointer, p1 > p2,
 * a negative penalty, p2 over the bound, a bad num_disparities, block_size, batch or shape, a short workspace) returns
 * SVO_ERR_INVALID with a message naming the argument and launches nothing. */
int svo_stereo_sgm_batch_dev(svo_ctx* ctx, const uint8_t* left, const uint8_t* right, int batch, int width, int height,
                             int row_stride, size_t image_stride, int num_disparities, int block_size, const svo_sgm_params* params,
                             void* workspace, size_t workspace_bytes, int16_t* disp16, uint16_t* cost16);
/* One pair, HOST pointers, synchronous; the work space is allocated and freed by the call.  cost16: width*height or NULL. */
int svo_stereo_sgm(svo_ctx* ctx, const uint8_t* left, const uint8_t* right, int width, int height, int row_stride,
                   int num_disparities, int block_size, const svo_sgm_params* params, int16_t* disp16, uint16_t* cost16);

/* ---------------------------------------------------------------- voxel map --
 * A device-resident sparse voxel grid: clouds (svo_cloud_point records on the device, in a camera frame) are fused into ONE
 * deduplicated world-frame map under a camera->world transform, keyframe by keyframe, and the occupied voxels come back as a
 * point list of the same record type (no reference counterpart; this is the project's own statement).  Every quantity is exact:
 * integers, or f64 operations in the stated order without contraction.
 *   Transform.  m12: 3 x 4 row-major f64 camera->world, 12 HOST doubles, passed to the kernel by value.
 *   Per record p = {x, y, z, tag}:
 *   1. Rejected iff !(p.z > 0.0f), or max_depth > 0 && p.z > max_depth (f32 comparisons on the camera-frame z; a NaN z fails the
 *      first test).
 *   2. For r = 0, 1, 2: w_r = m[r][0]*(double)x + m[r][1]*(double)y + m[r][2]*(double)z + m[r][3], f64 products summed left to
 *      right; q_r = w_r / (double)voxel_size.  Rejected iff any q_r fails q_r >= -1048576.0 && q_r < 1048576.0 (NaN, infinity,
 *      out of range).
 *   3. k_r = floor(q_r); key = (k_0 + 2^20) | (k_1 + 2^20) << 21 | (k_2 + 2^20) << 42, below 2^63, so EMPTY = ~0 is never a key.
 *      f_r = min((uint64)floor((q_r - k_r) * 65536.0), 65535) (the min matters: for a tiny negative q, q - floor(q) rounds to 1.0).
 *   4. Payload added to the voxel, four u64 words: ci += (1 << 40) | (tag >> 24) (count in bits 40..63, intensity sum in bits
 *      0..39); sx += f_0; sy += f_1; sz += f_2.  A voxel therefore holds at most 2^24 - 1 points: the CALLER's bound, not checked.
 *   Table.  Structure of arrays, cap = 2^capacity_log2 slots: keys[cap] u64, then ci, sx, sy, sz, each [cap] u64 (40 bytes per
 *      slot, 168 MB at the default).  Home slot h = fmix64(key) & (cap - 1) with fmix64(k): k ^= k >> 33; k *= 0xff51afd7ed558ccd;
 *      k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53; k ^= k >> 33.  Linear probing, at most SVO_VOXEL_MAX_PROBES probes, each a 64-bit
 *      atomic compare-and-swap of keys[h] from EMPTY to key whose RETURN value decides (EMPTY: claimed; key: found; anything else:
 *      next slot).  That rule is about launches that CLAIM slots (insert, copy); a launch that claims nothing (extraction, carve,
 *      render, removal) reads keys written by earlier launches on the same stream, and there a load may decide.  After SVO_VOXEL_MAX_PROBES foreign slots the record is dropped and counted: a full table costs a bounded time.
 *      The bound is part of the contract.
 *   Counters.  n_voxels (slots claimed), n_inserted, n_rejected, n_dropped (points); inserted + rejected + dropped = records given.
 *   Order independence.  While n_dropped == 0 the occupied slot set and every voxel's payload depend on no thread order (the set
 *      of cells occupied under linear probing does not depend on insertion order; integer sums commute); WHICH slot a key sits in
 *      is not defined.  Once n_dropped > 0 only this holds: every stored key is a key of some given record, every payload word is
 *      at most the true one, n_voxels is the number of stored keys, and the counter identity above.
 *   Extraction.  Every slot with key != EMPTY and count >= min_count becomes one svo_cloud_point: with c = (double)count,
 *      x = (float)(((double)k_0 + (double)sx / (c * 65536.0)) * (double)voxel_size), likewise y, z (the mean position inside the
 *      voxel); tag = count | (isum / count) << 24 (integer division; the count fits 24 bits by the bound above).  The output order
 *      is not defined.  counts = {n_total, n_stored = min(n_total, max_points)}; records behind n_stored are not written.
 *   Synchronisation.  Relaxed device-scope atomics only; no fence, no waiting on another workgroup or launch; everything on
 *      svo_stream(ctx), ordered by launch. */
typedef struct svo_voxel_map_params {
  float voxel_size;   /* finite, > 0; the units of the clouds (the baseline's) */
  int capacity_log2;  /* 8..28 */
  float max_depth;    /* <= 0: no bound on the camera-frame z */
} svo_voxel_map_params;
#define SVO_VOXEL_MAX_PROBES 64
typedef struct svo_voxel_map svo_voxel_map;
typedef struct svo_voxel_map_stats_t {
  uint64_t n_voxels, n_inserted, n_rejected, n_dropped;
} svo_voxel_map_stats_t;
/* voxel_size 0.1, capacity_log2 22, max_depth 0. */
int svo_voxel_map_default_params(svo_voxel_map_params* params);
/* Bytes of the table (what svo_voxel_map_download copies): 40 << capacity_log2.  Pure; SVO_ERR_INVALID and *bytes = 0 for
 * parameters svo_voxel_map_create refuses. */
int svo_voxel_map_bytes(const svo_voxel_map_params* params, size_t* bytes);
/* Allocates the table and clears it.  The map uses ctx's device and stream and must be destroyed before ctx. */
int svo_voxel_map_create(svo_ctx* ctx, const svo_voxel_map_params* params, svo_voxel_map** out);
void svo_voxel_map_destroy(svo_voxel_map* map);
/* Keys to EMPTY, payload and counters to 0; asynchronous. */
int svo_voxel_map_clear(svo_voxel_map* map);
/* n records at the DEVICE pointer `points` (4-byte aligned) inserted under m12; asynchronous, one launch.  n == 0 is a no-op. */
int svo_voxel_map_insert_dev(svo_voxel_map* map, const svo_cloud_point* points, int n, const double* m12);
/* pose7 = [qw qx qy qz tx ty tz], "world with respect to camera", X_cam = R(q) X_world + t (src/bundle_adjuster.hpp:50,
 * src/reprojection_factor.cpp:24-33) -> m12 = [R^T | -R^T t], i.e. X_world = R(q)^T (X_cam - t).  With s = 2 / (qw^2 + qx^2 +
 * qy^2 + qz^2) (so q need not be a unit quaternion):
 *   R = [1 - s(qy^2 + qz^2), s(qx qy - qw qz), s(qx qz + qw qy);
 *        s(qx qy + qw qz), 1 - s(qx^2 + qz^2), s(qy qz - qw qx);
 *        s(qx qz - qw qy), s(qy qz + qw qx), 1 - s(qx^2 + qy^2)],
 * m12[r][c] = R[c][r], m12[r][3] = -(R[0][r] t_0 + R[1][r] t_1 + R[2][r] t_2).  Pure host arithmetic (a zero quaternion gives
 * non-finite entries, under which every record is rejected). */
int svo_pose7_to_cam_to_world(const double* pose7, double* m12);
/* svo_pose7_to_cam_to_world, then svo_voxel_map_insert_dev. */
int svo_voxel_map_insert_pose7_dev(svo_voxel_map* map, const svo_cloud_point* points, int n, const double* pose7);
/* The four counters; synchronises the stream. */
int svo_voxel_map_stats(svo_voxel_map* map, svo_voxel_map_stats_t* stats);
/* Extraction into DEVICE memory, asynchronous: points: max_points records (may be NULL when max_points == 0); counts: 2 device
 * ints, zeroed on the stream before the launch.  min_count >= 1, max_points >= 0. */
int svo_voxel_map_extract_dev(svo_voxel_map* map, int min_count, svo_cloud_point* points, int max_points, int* counts);
/* Extraction into HOST memory, synchronous; points: `capacity` records (may be NULL when capacity == 0, which only counts). */
int svo_voxel_map_extract(svo_voxel_map* map, int min_count, svo_cloud_point* points, int capacity, int* n_total, int* n_stored);
/* Synchronous copy of the table in the layout above (keys, ci, sx, sy, sz); bytes >= svo_voxel_map_bytes.  What a caller
 * persists, and what gives the exact sums.  There is no upload.
 * Every entry above refuses a null pointer, bad parameters, n < 0, min_count < 1, max_points < 0 or a short download buffer with
 * SVO_ERR_INVALID and a message naming the argument (svo_last_error of the map's context); a refused call launches nothing. */
int svo_voxel_map_download(svo_voxel_map* map, void* host, size_t bytes);

/* Free-space carving: a keyframe's disparity map is evidence that the voxels it sees THROUGH are empty.  One launch over the
 * table, one thread per slot; disp16 is a tight width x height CV_16S map in sixteenths (FILTERED = -16) on the device, cam the
 * camera it was matched with (focal, cx, cy, baseline are read), w2c12 the 3 x 4 row-major f64 WORLD->CAMERA transform of that
 * keyframe (12 HOST doubles, passed to the kernel by value).  Every step is an integer or an f64 operation in the stated order,
 * without contraction:
 *   1. A slot is live iff key != EMPTY and count = ci >> 40 >= 1.  Other slots are skipped.
 *   2. World position, the extraction's mean before its cast to float:
 *      p_r = ((double)k_r + (double)s_r / ((double)count * 65536.0)) * (double)voxel_size.
 *   3. Camera position: c_r = m[r][0]*p_0 + m[r][1]*p_1 + m[r][2]*p_2 + m[r][3], summed left to right.
 *   4. Projection.  Not tested unless c_2 > 0.0.  u = focal*c_0 / c_2 + cx, v = focal*c_1 / c_2 + cy (multiply, divide, add);
 *      px = floor(u + 0.5), py = floor(v + 0.5).  Tested iff px >= radius && px <= width-1-radius && py >= radius &&
 *      py <= height-1-radius, compared in f64 (NaN and infinity fail).
 *   5. Window.  The (2 radius + 1)^2 values of disp16 around (px, py).  Any value <= 0 (filtered, or no disparity) is no
 *      evidence: the voxel is not carved.  Otherwise dmax is the window's maximum: the nearest surface any of these rays met,
 *      which keeps a depth edge from carving the neighbours of the background.
 *   6. Predicted disparity of the voxel in sixteenths: dv16 = (focal*baseline) / c_2 * 16.0.
 *   7. See-through iff (double)(dmax + margin16) < dv16 (strict).
 *   8. Carved iff see-through and not protected; protected means keep_count > 0 && count >= keep_count.  A carved slot gets
 *      ci = sx = sy = sz = 0 by plain stores (each thread writes its own slot only).  THE KEY STAYS: probe chains and "the
 *      CAS's return decides" are untouched, there are no tombstones, a later insert finds the key and starts the voxel again,
 *      n_voxels keeps meaning "slots claimed", and the extraction skips the slot because count < min_count.  Only a copy
 *      (below) gives such slots back.
 *   9. counts = {n_live, n_tested, n_carved}: 3 u64 on the device, zeroed on the stream before the launch, one relaxed
 *      atomicAdd per workgroup and non-zero counter; or NULL.
 *  10. SVO_ERR_INVALID with the argument named, and no launch, for: a null map, disp16, cam, w2c12 or params; radius outside
 *      0..3; margin16 outside 0..32767; keep_count < 0; width or height < 2 radius + 1 or beyond the context's limits;
 *      focal == 0 or baseline == 0.
 * The defaults (radius 1, margin16 8 = half a pixel of disparity, keep_count 0) are NOT tuned on real imagery: half a pixel is
 * above the quantisation and the noise of the synthetic scenes of the tests, whose own view carves nothing with them.
 * The pipeline never carves by itself: only the caller knows when a keyframe's pose is final. */
typedef struct svo_voxel_carve_params {
  int radius;     /* 0..3: half width of the window */
  int margin16;   /* 0..32767: sixteenths of disparity a voxel must lie in front of the seen surface */
  int keep_count; /* 0: off; > 0: voxels with at least this many points are never carved */
} svo_voxel_carve_params;
int svo_voxel_carve_default_params(svo_voxel_carve_params* params);
/* Asynchronous on svo_stream(ctx), one launch (and the counts' memset). */
int svo_voxel_map_carve_dev(svo_voxel_map* map, const int16_t* disp16, int width, int height, const svo_camera_info* cam,
                            const double* w2c12, const svo_voxel_carve_params* params, uint64_t* counts);
/* pose7 as svo_pose7_to_cam_to_world takes it -> m12 = [R | t] with the same R (s = 2 / |q|^2), i.e. X_cam = R(q) X_world + t:
 * m12[r][c] = R[r][c], m12[r][3] = t_r.  Pure host arithmetic. */
int svo_pose7_to_world_to_cam(const double* pose7, double* m12);
/* svo_pose7_to_world_to_cam, then svo_voxel_map_carve_dev. */
int svo_voxel_map_carve_pose7_dev(svo_voxel_map* map, const int16_t* disp16, int width, int height, const svo_camera_info* cam,
                                  const double* pose7, const svo_voxel_carve_params* params, uint64_t* counts);
/* disp16 in HOST memory, synchronous: upload, carve, counts[3] = {n_live, n_tested, n_carved} on the host (may be NULL). */
int svo_voxel_map_carve(svo_voxel_map* map, const int16_t* disp16, int width, int height, const svo_camera_info* cam,
                        const double* w2c12, const svo_voxel_carve_params* params, uint64_t* counts);
/* Copy of the live voxels (reclaim carved slots into a fresh table, cut a window out of a map, merge two maps): every slot of
 * src with key != EMPTY and count >= min_count (>= 1) - and, with box6 = {lo_0, lo_1, lo_2, hi_0, hi_1, hi_2} != NULL (6 HOST
 * doubles, not NaN), klo_r <= k_r <= khi_r for r = 0, 1, 2 with klo_r = floor(lo_r / (double)voxel_size), khi_r = floor(hi_r /
 * (double)voxel_size) computed on the host and compared as integers - is looked up or claimed in dst by the insert's own probe
 * loop, and its four words are added to dst's with the four atomicAdds: copying into a non-empty dst is a merge.  dst counters:
 * n_voxels += slots claimed, n_inserted += counts moved, n_dropped += counts that found no slot in SVO_VOXEL_MAX_PROBES probes
 * (then dst holds the overflow invariants of "Order independence").  src is only read.  Asynchronous, one launch.
 * SVO_ERR_INVALID and no launch for a null map, src == dst, maps of different contexts, voxel sizes that differ in a bit,
 * min_count < 1, a NaN in box6. */
int svo_voxel_map_copy_live_dev(svo_voxel_map* src, svo_voxel_map* dst, int min_count, const double* box6);

/* Voxel map render: what the map predicts for a camera at a pose, as a tight width x height CV_16S disparity map in sixteenths
 * (FILTERED = -16 where no voxel is seen) and a u8 intensity image: the formats of the dense track, so the view can carve another
 * map (svo_voxel_map_carve*), become the cloud of the visible surface (svo_disparity_cloud_batch_dev with the intensity image as
 * `left`), pass the speckle filter, or be subtracted from a keyframe's measured map.  cam: focal, cx, cy, baseline are read;
 * w2c12: WORLD->CAMERA, 12 HOST doubles, passed to the kernel by value.  Every step is an integer or an f64 operation in the stated
 * order, without contraction; steps 2-4 are the carve's:
 *   1. A slot qualifies iff key != EMPTY and count = ci >> 40 >= min_count (>= 1).  Carved slots have count 0: they never qualify.
 *   2. p_r = ((double)k_r + (double)s_r / ((double)count * 65536.0)) * (double)voxel_size.
 *   3. c_r = m[r][0]*p_0 + m[r][1]*p_1 + m[r][2]*p_2 + m[r][3], summed left to right.
 *   4. Not drawn unless c_2 > 0.0.  u = focal*c_0 / c_2 + cx, v = focal*c_1 / c_2 + cy; px = floor(u + 0.5), py = floor(v + 0.5).
 *   5. dv16 = (focal*baseline) / c_2 * 16.0 (the carve's step 6); d16 = floor(dv16 + 0.5).  Not drawn unless 1.0 <= d16 &&
 *      d16 <= 32767.0, compared in f64 (NaN and infinity fail).
 *   6. Footprint.  The voxel's cube of side voxel_size projects to a half width of h = focal*(double)voxel_size / c_2 * 0.5 pixels;
 *      r = min((double)max_radius, floor(h + 0.5)): the smallest half width whose 2r+1 pixels cover the 2h pixels between the means
 *      of neighbouring voxels of a surface that faces the camera.
 *   7. Drawn iff -r <= px && px <= width-1+r && -r <= py && py <= height-1+r, in f64.  Its pixels are all (x, y) with |x - px| <= r
 *      and |y - py| <= r, clipped to the image: a voxel whose centre is just outside still draws the part of its footprint inside.
 *   8. Z-buffer.  pix32 = (uint32)d16 << 8 | (uint32)(isum / count), isum the low 40 bits of ci; never 0.  Every pixel of the
 *      footprint gets pix[y*width + x] = max(pix[...], pix32) by a relaxed device-scope 32-bit atomicMax: the largest disparity (the
 *      nearest surface) wins, among equal disparities the larger mean intensity.  max commutes: the image depends on no thread
 *      order and on no slot placement.
 *   9. Resolve, a second launch on the same stream: pix == 0 gives disp16 = -16 and intensity = 0; otherwise disp16 = pix >> 8 and
 *      intensity = pix & 255.
 *  10. counts = {n_qualifying, n_drawn, n_splat, n_pixels}: 4 u64 on the device, or NULL.  n_splat: the sum over drawn voxels of
 *      their clipped footprint areas (the contract's number of max operations); n_pixels: pixels with pix != 0, counted by the
 *      resolve.  The workspace and the counts are zeroed on the stream before the first launch; one relaxed atomicAdd per
 *      workgroup and non-zero counter.
 *  11. SVO_ERR_INVALID with the argument named, and nothing launched, for: a null map, cam, w2c12, params, workspace or disp16;
 *      min_count < 1; max_radius outside 0..16; width or height < 1 or beyond the context's limits; focal or baseline not finite
 *      or <= 0; a workspace that is not 4-byte aligned.
 * workspace: svo_voxel_render_workspace_bytes(width, height) = 4*width*height bytes of device memory, one u32 per pixel (contents
 * before are meaningless, afterwards the z-buffer).  disp16: tight int16; intensity: tight u8 or NULL.  The resolve moves four
 * pixels per thread by vector accesses when workspace, disp16 and intensity are 16-, 8- and 4-byte aligned, and pixel by pixel
 * otherwise: the same bytes either way.
 * KNOWN PROPERTY: this is point splatting, not ray casting.  A surface seen at a grazing angle has voxel means more than 2r+1
 * pixels apart and shows holes, through which whatever lies behind is visible.
 * The defaults (min_count 1, max_radius 8) are NOT tuned on real imagery.  The pipeline never renders by itself. */
typedef struct svo_voxel_render_params {
  int min_count;  /* >= 1: voxels with fewer points are not drawn */
  int max_radius; /* 0..16: bound on the footprint's half width in pixels (0: one pixel per voxel) */
} svo_voxel_render_params;
int svo_voxel_render_default_params(svo_voxel_render_params* params);
/* 4*width*height; 0 for width or height < 1.  Pure. */
size_t svo_voxel_render_workspace_bytes(int width, int height);
/* DEVICE pointers, asynchronous on svo_stream(ctx): two memsets and two launches. */
int svo_voxel_map_render_dev(svo_voxel_map* map, int width, int height, const svo_camera_info* cam, const double* w2c12,
                             const svo_voxel_render_params* params, void* workspace, int16_t* disp16, uint8_t* intensity,
                             uint64_t* counts);
/* svo_pose7_to_world_to_cam, then svo_voxel_map_render_dev. */
int svo_voxel_map_render_pose7_dev(svo_voxel_map* map, int width, int height, const svo_camera_info* cam, const double* pose7,
                                   const svo_voxel_render_params* params, void* workspace, int16_t* disp16, uint8_t* intensity,
                                   uint64_t* counts);
/* HOST outputs, synchronous: the workspace and the device outputs are allocated and freed by the call.  intensity: width*height
 * bytes or NULL; counts: 4 u64 on the host or NULL. */
int svo_voxel_map_render(svo_voxel_map* map, int width, int height, const svo_camera_info* cam, const double* w2c12,
                         const svo_voxel_render_params* params, int16_t* disp16, uint8_t* intensity, uint64_t* counts);
/* Measurement aid: how the splat launch draws.  cooperative != 0: footprints with r > 1 are drawn by the whole wavefront in turn
 * (else every lane draws its own); precheck != 0: a plain load skips the atomic where the pixel already holds at least the value.
 * Neither can change a bit of the outputs.  Default: cooperative on, precheck off (DESIGN 7h gives the figures). */
int svo_voxel_render_set_mode(svo_voxel_map* map, int cooperative, int precheck);

/* Voxel map removal: a cloud taken back out of the map, the exact inverse of its insert, and the move of a cloud from one pose to
 * another (a keyframe whose pose bundle adjustment refined).  A voxel's payload is four integer sums and a record's contribution is
 * a pure function of the record's bytes, the matrix bits and voxel_size, so subtracting the same contribution undoes the insert bit
 * for bit, in any order.  Integers, or f64 operations in the stated order without contraction.  Inputs: the map, n records at a
 * DEVICE pointer (4-byte aligned), m12 (camera->world, 12 HOST doubles, by value), optional counts (4 u64 on the device, 8-byte
 * aligned, zeroed on the stream before the launch).
 *   1. Reject, transform, key and fractions are items 1-3 of the voxel map, word for word.  A record's contribution is the insert's:
 *      c = 1, i = tag >> 24, f_0, f_1, f_2.
 *   2. Find, never claim.  From the home slot fmix64(key) & (cap - 1), linear probing, at most SVO_VOXEL_MAX_PROBES slots:
 *      keys[h] == key: found; EMPTY: absent; anything else: next slot; after 64 foreign slots the key is absent.  A removal writes no
 *      key, and every key it reads was written by an earlier launch on the same stream: a load decides.  keys, n_voxels and the other
 *      three map counters are byte-identical after any removal (n_inserted keeps counting what was ever inserted).
 *   3. Saturating subtraction, per field.  Over a whole launch a voxel holding (count, isum, sx, sy, sz) whose found contributions sum
 *      to (C, I, F_0, F_1, F_2) ends with count' = max(0, count - C).  count' == 0: isum' = sx' = sy' = sz' = 0 - a voxel emptied by a
 *      removal is exactly a carved voxel: the key stays and a later insert starts it again.  Otherwise isum' = max(0, isum - I) and
 *      s_r' = max(0, s_r - F_r).  Successive saturating subtractions equal one saturating subtraction of the sum, and a count that
 *      reached 0 stays 0 for the rest of the launch: the result depends on no thread order, also where item 4 does not hold.
 *   4. Exact inverse.  If the removal has the record bytes, the m12 bits, the voxel_size and the max_depth of an earlier insert, that
 *      insert's n_dropped did not grow, and no carve has zeroed one of its voxels since, then afterwards every payload word is what
 *      the map would hold had that insert never happened, and n_short == 0 and n_missing == 0.
 *   5. counts = {n_removed, n_rejected, n_missing, n_short}, in points.  n_removed: records whose key was found; n_missing: key
 *      absent; removed + rejected + missing = n.  n_short: over all found contributions the part of C the count field no longer
 *      held, sum of c - min(c, count before that step), which is C - (count - count') per voxel in any order.  One relaxed atomicAdd
 *      per workgroup and non-zero counter.
 *   6. KNOWN PROPERTY.  A voxel that was carved, then refilled by other clouds, and only then has the old cloud removed loses mass that
 *      was not the old cloud's; n_short sees it only when the count runs out.  A per-voxel record of who contributed is what a hash
 *      of sums cannot hold.  The order of use that avoids it: update poses BEFORE carving with them (see the ledger below).
 *   7. SVO_ERR_INVALID with the argument named, nothing launched and the map usable afterwards: a null map, points (with n > 0), m12,
 *      from_m12 or to_m12 (pose7 for the pose entries); n < 0; points not 4-byte or counts not 8-byte aligned.  n == 0 is a no-op:
 *      nothing is launched and counts is not written.
 * Synchronisation as for the voxel map: relaxed device-scope atomics only, everything on svo_stream(ctx), ordered by launch. */
/* Asynchronous: the counts' memset and one launch. */
int svo_voxel_map_remove_dev(svo_voxel_map* map, const svo_cloud_point* points, int n, const double* m12, uint64_t* counts);
/* svo_pose7_to_cam_to_world, then svo_voxel_map_remove_dev. */
int svo_voxel_map_remove_pose7_dev(svo_voxel_map* map, const svo_cloud_point* points, int n, const double* pose7, uint64_t* counts);
/* svo_voxel_map_remove_dev with counts of its own, synchronous: counts[4] on the HOST (not NULL; all 0 for n == 0). */
int svo_voxel_map_remove_sync(svo_voxel_map* map, const svo_cloud_point* points, int n, const double* m12, uint64_t* counts);
/* The removal under from_m12, then the insert under to_m12: two launches on the stream; counts are the removal's.  When the two
 * matrices are equal in every bit nothing is launched, counts is not written, and the call succeeds.  There is no fused launch:
 * saturation does not commute with additions, so one launch would make the result depend on the thread order. */
int svo_voxel_map_move_dev(svo_voxel_map* map, const svo_cloud_point* points, int n, const double* from_m12, const double* to_m12,
                           uint64_t* counts);
/* svo_pose7_to_cam_to_world of both poses, then svo_voxel_map_move_dev. */
int svo_voxel_map_move_pose7_dev(svo_voxel_map* map, const svo_cloud_point* points, int n, const double* from_pose7,
                                 const double* to_pose7, uint64_t* counts);

/* Voxel map ledger: the clouds of the keyframes still in the bundle adjuster's window, kept on the device with the pose each was
 * inserted under, so that "this keyframe's pose is now X" is one call.  The ledger owns a copy of every held cloud (a pipeline's
 * cloud is valid only until the next process call) and remembers the matrix bits of its insert, which the removal needs.
 * Order of use: insert each new keyframe's cloud, update the held ones whenever newer poses exist, retire a keyframe when it leaves
 * the window, and carve only AFTER updating (item 6 above).  create is the only allocation; every other entry is asynchronous on
 * the map's stream, without synchronisation or device allocation.  Refusals are SVO_ERR_INVALID with the argument named and nothing
 * launched. */
typedef struct svo_voxel_ledger_params {
  int max_keyframes; /* >= 1: clouds held at once */
  int max_points;    /* >= 1: records per cloud */
} svo_voxel_ledger_params;
typedef struct svo_voxel_ledger svo_voxel_ledger;
/* Device bytes a ledger allocates: 16 * max_keyframes * max_points.  Pure; SVO_ERR_INVALID and *bytes = 0 for refused parameters. */
int svo_voxel_ledger_bytes(const svo_voxel_ledger_params* params, size_t* bytes);
/* Destroy the ledger before its map. */
int svo_voxel_ledger_create(svo_voxel_map* map, const svo_voxel_ledger_params* params, svo_voxel_ledger** out);
void svo_voxel_ledger_destroy(svo_voxel_ledger* ledger);
/* Copies the n records device->device into a free slot, inserts the copy into the map under pose7 and records pose7 and the matrix
 * computed from it.  Refused when the id is held, when no slot is free, when n > max_points or n < 0. */
int svo_voxel_ledger_insert_pose7_dev(svo_voxel_ledger* ledger, int64_t id, const svo_cloud_point* points, int n, const double* pose7);
/* svo_voxel_map_move_dev of the held copy from the recorded matrix to pose7's, then records pose7.  counts: the removal's, or NULL.
 * An unknown id is refused. */
int svo_voxel_ledger_update_pose7(svo_voxel_ledger* ledger, int64_t id, const double* pose7, uint64_t* counts);
/* The pose is final: the map is untouched and the slot is free for the next insert (safe: everything is ordered on one stream). */
int svo_voxel_ledger_retire(svo_voxel_ledger* ledger, int64_t id);
/* Removes the held copy from the map (svo_voxel_map_remove_dev under the recorded matrix) and frees the slot. */
int svo_voxel_ledger_remove(svo_voxel_ledger* ledger, int64_t id, uint64_t* counts);
/* The held ids in ascending order: at most `capacity` are written (ids may be NULL when capacity == 0), *n is how many are held. */
int svo_voxel_ledger_ids(svo_voxel_ledger* ledger, int64_t* ids, int capacity, int* n);
/* What is held under id: the recorded pose7 (7 doubles), the record count and the DEVICE pointer of the copy; each may be NULL. */
int svo_voxel_ledger_get(svo_voxel_ledger* ledger, int64_t id, double* pose7, int* n, const svo_cloud_point** points);

/* Voxel map align: the map is asked where a new cloud fits (scan-to-map refinement of a keyframe's pose BEFORE its cloud is
 * inserted).  One launch matches every record of the cloud with the nearest voxel mean around it and reduces the normal equations
 * of a point-to-point pose increment to 21 integers; a small host loop solves the 6 x 6 system and repeats.  Every step is an
 * integer operation or an f64 operation in the written order, without contraction.  Inputs of both entries: the map, n records at
 * a DEVICE pointer (4-byte aligned, as for the insert), a camera->world transform m (12 HOST doubles by value, the insert's
 * matrix) and svo_voxel_align_params.  Per record p = {x, y, z, tag}:
 *   1. Rejected (n_rejected) iff item 1 of the voxel map rejects it (!(z > 0.0f), or max_depth > 0 && z > max_depth), or any of
 *      |x|, |y|, |z| fails < 1024.0f (f32; a NaN fails), or, with w_r and q_r exactly as item 2 of the voxel map, any q_r fails
 *      q_r >= -1048575.0 && q_r < 1048575.0: one voxel inside the key range, so every neighbour has a key.
 *   2. Candidates.  k_r = floor(q_r); the candidates are the voxels k + (i, j, l) with |i|, |j|, |l| <= reach (reach 0 or 1: 1 or
 *      27 voxels), each with the voxel map's key of its indices.  Each is looked up by item 2 of "Voxel map removal": home slot,
 *      linear probing, a plain load decides; keys[h] == key is found, EMPTY is absent, and after SVO_VOXEL_MAX_PROBES foreign
 *      slots the key is absent.  A found slot QUALIFIES iff count = ci >> 40 >= min_count (>= 1): carved slots never qualify.
 *      Nothing is ever claimed or written to the table: its bytes and the map's counters are the same afterwards.
 *   3. Nearest candidate.  A qualifying candidate k' has the mean mu_r = ((double)k'_r + (double)s_r / ((double)count * 65536.0))
 *      * (double)voxel_size (the render's rule 2).  e_r = w_r - mu_r; d2 = e_0*e_0 + e_1*e_1 + e_2*e_2, summed left to right.  The
 *      MATCH is the qualifying candidate with the smallest d2, and among equal d2 the one with the smallest key (as u64).  No
 *      qualifying candidate: n_unmatched.  d2 > (double)max_dist * (double)max_dist: n_far (equality still matches).
 *   4. A match's contribution.  Residual in the camera frame: c_r = m[0][r]*e_0 + m[1][r]*e_1 + m[2][r]*e_2, left to right;
 *      P = ((double)x, (double)y, (double)z).  The model is c(xi) ~ c + v + omega x P for a pose increment xi = (v, omega) applied
 *      on the camera side, m' = m [I + [omega]x | v].  Its normal equations need 17 sums; every non-count term is quantised PER
 *      RECORD by Q_S(t) = (int64)floor(t*S + 0.5) (multiply, add, floor, convert) and the terms are added as 64-bit integers:
 *        word 0      N, the number of matches
 *        words 1-3   Q_16(P_0), Q_16(P_1), Q_16(P_2)                                             S = 2^16
 *        words 4-9   Q_16(P_0*P_0), Q_16(P_0*P_1), Q_16(P_0*P_2), Q_16(P_1*P_1), Q_16(P_1*P_2), Q_16(P_2*P_2)   S = 2^16
 *        words 10-12 Q_28(c_0), Q_28(c_1), Q_28(c_2)                                             S = 2^28
 *        words 13-15 Q_28(P_1*c_2 - P_2*c_1), Q_28(P_2*c_0 - P_0*c_2), Q_28(P_0*c_1 - P_1*c_0)   (product, product, difference)
 *        word 16     Q_28(c_0*c_0 + c_1*c_1 + c_2*c_2), left to right: the cost
 *      Integer sums commute: the words and the counts depend on no thread order and on no slot placement.
 *   5. Bounds.  n <= 2^20; max_dist finite and in (0, 8]; |P_i| < 1024 by rule 1; the 3 x 3 part of m is a rotation (the CALLER's
 *      bound, not checked: with another matrix the words of rule 4 are not defined; nothing faults).  Then |c| = |e| <= 8 and
 *      |P| < 1774, so the largest term is |P x c| * 2^28 < 2^14 * 2^28 and no word exceeds 2^20 * 2^42 = 2^62 < 2^63 (the
 *      others: P_i P_j * 2^16 < 2^36, cost * 2^28 <= 2^34, P_i * 2^16 < 2^26, each times 2^20).
 *   6. sums: 32 int64 on the device, 8-byte aligned.  Words 0-16 as above; words 17-20 = {n_matched, n_rejected, n_unmatched,
 *      n_far}, whose sum is n (word 0 == word 17); words 21-31 are zero.  sums is zeroed on the stream before the launch; one
 *      relaxed atomicAdd per workgroup and non-zero word.
 * The host loop (svo_voxel_map_align; every step is +, -, *, / or sqrt on doubles in the written order, so a restatement in
 * another language gives the same bits).  pose7 is in the project's convention, X_cam = R(q) X_world + t:
 *   a. In.  s = sqrt(qw*qw + qx*qx + qy*qy + qz*qz); the camera->world quaternion is u = (qw/s, -qx/s, -qy/s, -qz/s); with
 *      R = R(u) by the rule of svo_pose7_to_cam_to_world (row-major R[3r + c]) the camera->world translation is
 *      T_r = -(R[3r]*t_0 + R[3r+1]*t_1 + R[3r+2]*t_2).
 *   b. Per iteration: R = R(u) by that rule, m[r][c] = R[3r + c], m[r][3] = T_r; one svo_voxel_map_align_sums_dev under m and a
 *      copy of the 32 words to the host.  n_matched < min_matches ends with SVO_VOXEL_ALIGN_TOO_FEW.
 *   c. H (symmetric 6 x 6, rows and columns 0-2 for v, 3-5 for omega) and g from the integers, each word converted to double and
 *      divided by its S (N by none): with A_i = word(1+i)/2^16, B = words 4-9 /2^16, H_vv = N I; H_v,omega = -[A]x, that is
 *      H[0][4] = A_2, H[0][5] = -A_1, H[1][3] = -A_2, H[1][5] = A_0, H[2][3] = A_1, H[2][4] = -A_0; H_omega,omega = (B_00 + B_11 +
 *      B_22) I - B, written H[3][3] = B_11 + B_22, H[4][4] = B_00 + B_22, H[5][5] = B_00 + B_11, off-diagonal H[3+i][3+j] = -B_ij;
 *      g = (words 10-12, words 13-15) / 2^28.
 *   d. Solve H xi = -g by an unpivoted Cholesky factorisation H = L L^T: for j = 0..5: d = H[j][j]; for k = 0..j-1: d = d -
 *      L[j][k]*L[j][k]; a pivot d that fails d > 0 && d <= DBL_MAX ends with SVO_VOXEL_ALIGN_DEGENERATE; L[j][j] = sqrt(d); for
 *      i = j+1..5: s = H[i][j]; for k = 0..j-1: s = s - L[i][k]*L[j][k]; L[i][j] = s / L[j][j].  Forward, i = 0..5: s = -g_i; for
 *      k = 0..i-1: s = s - L[i][k]*y_k; y_i = s / L[i][i].  Backward, i = 5..0: s = y_i; for k = i+1..5: s = s - L[k][i]*xi_k;
 *      xi_i = s / L[i][i].
 *   e. Update, with R still the matrix of step b: T_r = T_r + (R[3r]*v_0 + R[3r+1]*v_1 + R[3r+2]*v_2); b_i = omega_i / 2;
 *      u' = u (x) (1, b): w = u_0 - u_1*b_0 - u_2*b_1 - u_3*b_2; x = u_1 + u_0*b_0 + u_2*b_2 - u_3*b_1; y = u_2 + u_0*b_1 - u_1*b_2 +
 *      u_3*b_0; z = u_3 + u_0*b_2 + u_1*b_1 - u_2*b_0, each left to right; a = (w, x, y, z) / sqrt(w*w + x*x + y*y + z*z); then one first-order
 *      correction of the norm: h = (1 - (a_0*a_0 + a_1*a_1 + a_2*a_2 + a_3*a_3)) / 2, u_i = a_i + a_i*h.
 *   f. Stop SVO_VOXEL_ALIGN_CONVERGED when v_0*v_0 + v_1*v_1 + v_2*v_2 < (double)eps_t*(double)eps_t and the same of omega <
 *      (double)eps_r*(double)eps_r (both strict); else SVO_VOXEL_ALIGN_MAX_ITERS after max_iters iterations.
 *   g. Out.  No step taken: pose7_out = pose7_in, bit for bit.  Otherwise q = (u_0, -u_1, -u_2, -u_3) and, with R = R(u),
 *      t_r = -(R[r]*T_0 + R[3 + r]*T_1 + R[6 + r]*T_2).  pose7_out is written for every status.
 * Refusals: SVO_ERR_INVALID with the argument named, nothing launched, outputs untouched, in this order: a null map; n < 0;
 * n > 2^20; a null matrix or pose7 (pose7_in, then pose7_out, then result for the loop); null params; min_count < 1; reach outside
 * 0..1; max_dist not finite or outside (0, 8]; max_iters < 1; min_matches < 6; eps_t, then eps_r, not finite or negative; null
 * sums; sums not 8-byte aligned; and with n > 0 null points, then points not 4-byte aligned.
 * Order of use: align a keyframe's cloud BEFORE inserting it (a map that already holds the cloud pulls it to where it is), then
 * insert it (or svo_voxel_ledger_insert_pose7_dev) under the refined pose.  The pipeline never aligns by itself.
 * Synchronisation as for the voxel map: relaxed device-scope atomics only, no fence, everything on svo_stream(ctx). */
typedef struct svo_voxel_align_params {
  int min_count;   /* >= 1: voxels with fewer points are no candidates */
  int reach;       /* 0 or 1: the record's own voxel, or the 27 around it */
  float max_dist;  /* finite, in (0, 8]: matches farther than this (map units) are n_far */
  int max_iters;   /* >= 1 */
  int min_matches; /* >= 6 */
  float eps_t;     /* finite, >= 0: the stop rule's bound on |v| (map units) */
  float eps_r;     /* finite, >= 0: the stop rule's bound on |omega| (radians) */
} svo_voxel_align_params;
enum { SVO_VOXEL_ALIGN_CONVERGED = 0, SVO_VOXEL_ALIGN_MAX_ITERS = 1, SVO_VOXEL_ALIGN_TOO_FEW = 2, SVO_VOXEL_ALIGN_DEGENERATE = 3 };
#define SVO_VOXEL_ALIGN_WORDS 32
#define SVO_VOXEL_ALIGN_MAX_POINTS (1 << 20)
typedef struct svo_voxel_align_result {
  int status;          /* SVO_VOXEL_ALIGN_* */
  int iterations;      /* launches of the sums */
  int64_t first_matched, last_matched; /* n_matched of the first and of the last iteration */
  int64_t first_cost, last_cost;       /* word 16 of the first and of the last iteration */
  double xi[6];        /* the last increment (v, omega); zeros if no step was taken */
} svo_voxel_align_result;
/* min_count 1, reach 1, max_dist = 2 * voxel_size (at most 8), max_iters 10, min_matches 64, eps_t = voxel_size / 100, eps_r = 1e-5.
 * NOT tuned on real imagery.  Pure; SVO_ERR_INVALID for null params or a voxel_size that is not finite and > 0. */
int svo_voxel_align_default_params(float voxel_size, svo_voxel_align_params* params);
/* Asynchronous on svo_stream(ctx): one memset of sums and one launch, one "voxel_align" profile bracket.  n == 0 zeroes sums and
 * launches nothing more (points may then be NULL). */
int svo_voxel_map_align_sums_dev(svo_voxel_map* map, const svo_cloud_point* points, int n, const double* c2w12,
                                 const svo_voxel_align_params* params, int64_t* sums);
/* svo_pose7_to_cam_to_world, then svo_voxel_map_align_sums_dev. */
int svo_voxel_map_align_sums_pose7_dev(svo_voxel_map* map, const svo_cloud_point* points, int n, const double* pose7,
                                       const svo_voxel_align_params* params, int64_t* sums);
/* The host loop above, synchronous: DEVICE points; pose7_in, pose7_out (7 doubles each, may be the same array) and result on the
 * HOST.  The sums live in the context's scratch: nothing is allocated. */
int svo_voxel_map_align(svo_voxel_map* map, const svo_cloud_point* points, int n, const double* pose7_in,
                        const svo_voxel_align_params* params, double* pose7_out, svo_voxel_align_result* result);

/* Voxel map normals: one launch gives every voxel a surface normal and a curvature from the means of the 27 voxels around it, into
 * a side array of the CALLER's with one 16-byte record per slot, indexed by slot.  Slots never move and keys stay, so an index stays
 * valid across later inserts; only the values go stale, and the caller runs the launch again after inserts, removals or a carve.
 * Every record of the array is written by every call; no byte of the table and no map counter changes.  Every step is an integer
 * operation or an f64 operation in the written order, without contraction.  Per slot:
 *   1. Centre.  A slot is a centre iff its key is not EMPTY and count = ci >> 40 >= min_count (>= 1).  Any other slot gets the
 *      record {0, 0, 0, -1.0f}.
 *   2. Candidates.  With k the centre's indices, the 27 voxels k + (i, j, l), |i|, |j|, |l| <= 1, candidate c = (i + 1) + 3 (j + 1) +
 *      9 (l + 1) (the align's order; c = 13 is the centre).  A candidate one of whose indices leaves [-2^20, 2^20) has no key and is
 *      absent: the centre, unlike an align record, may sit at the edge of the key range.  Each other candidate is looked up by item
 *      2 of "Voxel map removal": home slot, linear probing, a plain load decides, absent after SVO_VOXEL_MAX_PROBES foreign slots;
 *      nothing is claimed.  A found candidate TAKES PART iff its count >= min_count; the centre always takes part.
 *   3. Integer moments.  Per participant and axis r, with o = (i, j, l) its offset and (s_0, s_1, s_2) = (sx, sy, sz) of its slot:
 *      g_r = o_r * 65536 + s_r div count (exact floor division; the mean in 65536ths of a voxel relative to the centre's voxel,
 *      -65536 <= g_r < 131072).  N = the number of participants; S1_r = sum g_r; S2_rs = sum g_r * g_s (r <= s); C_rs = N * S2_rs -
 *      S1_r * S1_s in int64 (each product is below 2^44).  Every voxel counts once, not once per point.  C is the covariance of the
 *      means scaled by 65536^2 N^2; it depends on no slot placement and on no thread order.
 *   4. Eigenvectors.  a = (double)C (symmetric, a_rs = a_sr), V = I (3 x 3).  Exactly 4 sweeps over (p, q) = (0, 1), (0, 2), (1, 2),
 *      with r the third index.  Per pair: skipped iff a_pq == 0.0; else
 *        th = (a_qq - a_pp) / (2.0 * a_pq);  t = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
 *        c = 1.0 / sqrt(t * t + 1.0);  s = t * c;
 *        x = t * a_pq;  a_pp = a_pp - x;  a_qq = a_qq + x;  a_pq = 0.0;
 *        y = a_rp, z = a_rq:  a_rp = c * y - s * z;  a_rq = s * y + c * z;
 *        for k = 0, 1, 2: y = V[k][p], z = V[k][q]:  V[k][p] = c * y - s * z;  V[k][q] = s * y + c * z.
 *      Only + - * / and sqrt; a th * th that overflows gives t = 0 by IEEE rules (th is never a NaN: a_pq != 0 and finite).
 *   5. Validity.  lambda_i = a_ii.  lo = the lowest index with the smallest lambda; mid = of the other two indices the one with
 *      the smaller lambda (the lower index if equal).  tr = lambda_0 + lambda_1 + lambda_2, left to right.  Tested in this order,
 *      the first failing test counts: N >= min_neighbours (else n_few; 3 <= min_neighbours <= 27); lambda_mid > 0.0 (else
 *      n_collinear: the means lie on a line or in a point); max(lambda_lo, 0.0) <= (double)max_curvature * tr (else n_curved).
 *      An invalid centre gets {0, 0, 0, -1.0f}.
 *   6. Output of a valid centre.  n = column lo of V; with m the lowest index of the largest fabs(n_i), n is negated iff n_m < 0.0;
 *      then each component is converted to f32.  curvature = (float)(max(lambda_lo, 0.0) / tr), in [0, 1/3].  A valid normal is
 *      never all zero: the zero vector is what "no normal" means to every reader.
 *   7. counts: 8 u64 on the device, 8-byte aligned, or NULL: {n_centres, n_valid, n_few, n_collinear, n_curved, 0, 0, 0} with
 *      n_centres = n_valid + n_few + n_collinear + n_curved.  Zeroed on the stream before the launch; combined per wavefront, then
 *      one relaxed atomicAdd per workgroup and non-zero word.
 * Refusals: SVO_ERR_INVALID with the argument named, nothing launched, outputs untouched, in this order: a null map; null params;
 * min_count < 1; min_neighbours outside 3..27; max_curvature not finite or outside (0, 1]; null normals; normals not 16-byte
 * aligned; counts not 8-byte aligned.
 * Order of use: after the last insert / update / carve and before whoever reads the normals.
 * Synchronisation as for the voxel map: relaxed device-scope atomics only (the counts), no fence, everything on svo_stream(ctx). */
typedef struct svo_voxel_normal { float nx, ny, nz, curvature; } svo_voxel_normal; /* 16 bytes; {0, 0, 0, -1}: no normal */
typedef struct svo_voxel_normals_params {
  int min_count;       /* >= 1: voxels with fewer points are neither centres nor neighbours */
  int min_neighbours;  /* 3..27: participants (the centre included) a normal needs */
  float max_curvature; /* finite, in (0, 1]: lambda_lo / trace above this is no surface; 1 refuses nothing */
} svo_voxel_normals_params;
#define SVO_VOXEL_NORMALS_COUNTS 8
/* min_count 1, min_neighbours 5, max_curvature 1.0f.  NOT tuned on real imagery.  Pure; SVO_ERR_INVALID for null params. */
int svo_voxel_normals_default_params(svo_voxel_normals_params* params);
/* Bytes of the side array: 16 << capacity_log2.  Pure; SVO_ERR_INVALID and *bytes = 0 for parameters svo_voxel_map_create refuses. */
int svo_voxel_map_normals_bytes(const svo_voxel_map_params* params, size_t* bytes);
/* Asynchronous on svo_stream(ctx): the counts' memset (if any) and one launch, one "voxel_normals" profile bracket.  normals: DEVICE,
 * svo_voxel_map_normals_bytes bytes. */
int svo_voxel_map_normals_dev(svo_voxel_map* map, const svo_voxel_normals_params* params, svo_voxel_normal* normals, uint64_t* counts);
/* svo_voxel_map_normals_dev into device memory of its own, copied to the HOST; synchronous; allocates and frees.  host_normals:
 * one record per slot (any alignment); host_counts: 8 words, or NULL. */
int svo_voxel_map_normals(svo_voxel_map* map, const svo_voxel_normals_params* params, svo_voxel_normal* host_normals,
                          uint64_t* host_counts);

/* Voxel map align, plane form: the align with the distance ALONG THE MATCHED VOXEL'S NORMAL as its residual.  A point-to-mean
 * residual holds a cloud along a plane only as well as the two samplings agree; this one lets it slide.  `normals` is the DEVICE
 * array svo_voxel_map_normals_dev wrote for this map (one record per slot; stale values are the caller's affair).
 * svo_voxel_align_params and svo_voxel_align_result are the align's.  Rules 1-3 of "Voxel map align" hold word for word (rejection,
 * candidates, the nearest qualifying mean, ties, n_far): the match is chosen BEFORE its normal is looked at.
 *   4'. A match's contribution.  With s the matched slot: nn = ((double)normals[s].nx, (double).ny, (double).nz).  If all three
 *      are zero the record is counted in n_no_normal and contributes nothing.  Otherwise, with e_r = w_r - mu_r (world frame) and
 *      P as in rule 4:
 *        r   = nn_0*e_0 + nn_1*e_1 + nn_2*e_2, left to right;
 *        a_c = m[0][c]*nn_0 + m[1][c]*nn_1 + m[2][c]*nn_2, left to right: the normal in the camera frame;
 *        b   = P x a: b_0 = P_1*a_2 - P_2*a_1, b_1 = P_2*a_0 - P_0*a_2, b_2 = P_0*a_1 - P_1*a_0 (product, product, difference).
 *      The model is r(xi) ~ r + a.v + b.omega for the same camera-side increment, so the Jacobian row is j = (a_0, a_1, a_2, b_0,
 *      b_1, b_2).  Every term is quantised per record by Q_S and added as a 64-bit integer:
 *        word 0       N, the contributing matches
 *        words 1-21   Q_S(j_i * j_k), i <= k, row-major over the upper triangle (word 1 + 6 i - i (i - 1) / 2 + (k - i));
 *                     S = 2^40 for i, k < 3; 2^30 for i < 3 <= k; 2^20 for i, k >= 3
 *        words 22-24  Q_36(a_i * r)
 *        words 25-27  Q_28(b_i * r)
 *        word 28      Q_28(r * r): the cost
 *        words 29-33  n_matched (= word 0), n_rejected, n_unmatched, n_far, n_no_normal; their sum is n
 *        words 34-39  zero
 *   5'. Bounds.  n <= 2^20; |P| < 1774; |nn| <= 1.0001 (the CALLER's bound, as the rotation is; the normals launch meets it);
 *      |e| <= 8.  Then a_i a_k <= 1.0003 and S = 2^40 gives less than 2^41; |a_i b_k| < 2^11 and S = 2^30 gives less than 2^41;
 *      |b_i b_k| < 2^22 and S = 2^20 gives less than 2^42; |a_i r| < 2^4 and S = 2^36 gives less than 2^40; |b_i r| < 2^14 and
 *      S = 2^28 gives less than 2^42; r*r <= 65 and S = 2^28 gives less than 2^35.  Every term times its S stays below 2^43 and no
 *      word exceeds 2^63.
 *   6'. sums: SVO_VOXEL_ALIGN_PLANE_WORDS int64 on the device, 8-byte aligned, zeroed on the stream before the launch; one relaxed
 *      atomicAdd per workgroup and non-zero word.
 * The host loop (svo_voxel_map_align_plane): steps a, b, d, e, f and g of the align's loop as they are, over these sums.  Step c':
 * H[i][k] = H[k][i] = (double)word(i, k) / S(i, k); g_i = (double)word(22 + i) / 2^36 for i < 3 and (double)word(22 + i) / 2^28 for
 * i >= 3.  SVO_VOXEL_ALIGN_TOO_FEW tests word 29; first_cost and last_cost are word 28, first_matched and last_matched word 29.  A
 * scene that does not hold all six freedoms (one plane; two planes leave the shift along their common line free only up to what
 * the match distance adds) ends SVO_VOXEL_ALIGN_DEGENERATE when a pivot fails, and is otherwise NOT held along its free directions:
 * the residual sees no motion inside a plane.
 * Refusals: the align's list in the align's order, with "null normals, then normals not 16-byte aligned" directly after the null map.
 * Order of use: svo_voxel_map_normals_dev after the map's last change, then this, then the cloud's own insert. */
#define SVO_VOXEL_ALIGN_PLANE_WORDS 40
/* Asynchronous on svo_stream(ctx): one memset of sums and one launch, one "voxel_align_plane" profile bracket.  n == 0 zeroes sums
 * and launches nothing more. */
int svo_voxel_map_align_plane_sums_dev(svo_voxel_map* map, const svo_voxel_normal* normals, const svo_cloud_point* points, int n,
                                       const double* c2w12, const svo_voxel_align_params* params, int64_t* sums);
/* svo_pose7_to_cam_to_world, then svo_voxel_map_align_plane_sums_dev. */
int svo_voxel_map_align_plane_sums_pose7_dev(svo_voxel_map* map, const svo_voxel_normal* normals, const svo_cloud_point* points, int n,
                                             const double* pose7, const svo_voxel_align_params* params, int64_t* sums);
/* The host loop, synchronous; the 40 words live in the context's scratch: nothing is allocated. */
int svo_voxel_map_align_plane(svo_voxel_map* map, const svo_voxel_normal* normals, const svo_cloud_point* points, int n,
                              const double* pose7_in, const svo_voxel_align_params* params, double* pose7_out,
                              svo_voxel_align_result* result);

/* Voxel map locate: the coarse stage in front of the align.  The align's basin is one voxel wide; this searches a box
 * of whole-voxel shifts and a fan of turns about one world axis for the pose under which most records of a cloud land in live
 * voxels, and hands the peak to the align.  Three parts: a dense bit volume of the map, the scores, and a host loop.  Integer work
 * throughout: a restatement in another language gives the same words.
 *
 * Occupancy volume (svo_voxel_map_occupancy_dev; also of use alone, for 3D collision tests).  Inputs: min_count >= 1; origin[3],
 * int32 voxel indices, each in [-2^20, 2^20); dims[3] = (d0, d1, d2), each in 1..2048, d0 a multiple of 64, d0*d1*d2 <= 2^30;
 * bits, DEVICE, 8-byte aligned, d0*d1*d2/8 bytes (svo_voxel_occupancy_bytes); counts, 2 DEVICE u32, 4-byte aligned.
 *   The voxel with indices i has j_r = i_r - origin_r and is INSIDE iff 0 <= j_r < d_r for all r.  Its bit number is
 *   B = j_0 + d0*(j_1 + d1*j_2), in the little-endian u64 word B >> 6 at bit B & 63.  The bit is 1 iff a slot holds that key and
 *   ci >> 40 >= min_count; carved slots are 0.  counts = {n_inside, n_outside} over the qualifying slots.  One memset of the volume
 *   and one of the counts, then one walk over the table with one thread per slot: a load decides, nothing is claimed, the bits are
 *   set by relaxed atomicOr and the counts added by relaxed atomicAdd (one per workgroup and non-zero count).  No byte of the table
 *   and no map counter changes.  Profile tag "voxel_occupancy".
 *   Refusals, in this order: a null map; min_count < 1; null origin; an origin_r outside [-2^20, 2^20); null dims; a d_r outside
 *   1..2048; d0 not a multiple of 64; d0*d1*d2 > 2^30; null bits; bits not 8-byte aligned; null counts; counts not 4-byte aligned.
 *
 * Scores (svo_voxel_map_locate_scores_dev).  Inputs: the map (read for voxel_size and max_depth ONLY: the table is not touched);
 * bits, origin, dims as above; n <= 2^20 records at a DEVICE pointer; K camera->world matrices, 1 <= K <= 63, as K*12 HOST doubles
 * (they travel as kernel arguments, at most 32 candidates per launch: K > 32 takes two score launches); box[3] = (r0, r1, r2), each
 * in 0..16, S_r = 2 r_r + 1; hits, DEVICE u32, K*S0*S1*S2 words, 4-byte aligned; best, K DEVICE svo_voxel_locate_best, 8-byte
 * aligned.  Per candidate k and record:
 *   1. Rejected (n_rejected[k] = n - n_used[k]) iff item 1 of the voxel map rejects it, or any of |x|, |y|, |z| fails < 1024.0f, or,
 *      with w_r and q_r exactly as item 2 of the voxel map under m_k, any q_r fails q_r >= -1048560.0 && q_r < 1048560.0: sixteen
 *      voxels inside the key range, whatever the box.
 *   2. j_r = floor(q_r) - origin_r.  A record that is not rejected counts in n_used[k], and in n_inside[k] iff j is inside.
 *   3. For every shift s with |s_r| <= r_r, c = j + s.  The record is a HIT iff c is inside the volume and its bit is 1; a c outside
 *      is never a hit.  hits[k*S0*S1*S2 + (s_2 + r2)*S1*S0 + (s_1 + r1)*S0 + (s_0 + r0)] is the number of hits: records count with
 *      multiplicity, at most 2^20.  Shift s means the cloud moved by s * voxel_size in the world.
 *   4. best[k] = {hits_max, s0, s1, s2, n_used, n_inside, index, 0}: hits_max the largest score of k, index the SMALLEST linear
 *      index inside k's block that holds it, s that index's shift.  All scores zero: index 0.
 *   hits and best are written in full by every call; n == 0 zeroes hits and writes the all-zero best with shift (-r0, -r1, -r2).
 *   Integer sums commute: nothing depends on thread order.  Relaxed device-scope atomics only, no fence, no waiting on another
 *   workgroup.  Profile tag "voxel_locate": one bracket over the memsets, the score launches and the best launch.
 *   Refusals, in this order: a null map; n < 0; n > 2^20; null mats; K outside 1..63; null box; a box_r outside 0..16; the origin
 *   and dims refusals above; null bits; bits not 8-byte aligned; null hits; hits not 4-byte aligned; null best; best not 8-byte
 *   aligned; and with n > 0 null points, then points not 4-byte aligned.
 *
 * The host loop (svo_voxel_map_locate; host/voxel_locate.h; only + - * / and sqrt on doubles in the written order, and NO
 * trigonometric function):
 *   a. In.  u, T from pose7_in by the align's step a.
 *   b. Candidates.  K = 2 n_turn + 1; candidate k has j = k - n_turn and b = ((double)j * (double)turn_step) / 2.  a = (1, b e_axis)
 *      / sqrt(1 + b*b), that is a_0 = 1 / nrm, a_axis = b / nrm, the other two 0.  u_k = a (x) u, the turn on the WORLD side, about
 *      the world axis through the camera centre: w = a_0*u_0 - a_1*u_1 - a_2*u_2 - a_3*u_3; x = a_0*u_1 + a_1*u_0 + a_2*u_3 - a_3*u_2;
 *      y = a_0*u_2 - a_1*u_3 + a_2*u_0 + a_3*u_1; z = a_0*u_3 + a_1*u_2 - a_2*u_1 + a_3*u_0, each left to right; then the align's
 *      normalisation with its first-order correction (step e).  m_k = [R(u_k) | T].  The angle of candidate k is 2 atan(b), NOT
 *      j * turn_step: the two differ by a factor 1 - b*b/3 + ..., 0.1 % at the default fan's end.
 *   c. Volume.  origin_r = (int)floor(T_r / (double)voxel_size) - d_r / 2 (integer division).  Refused with SVO_ERR_INVALID if a
 *      floor is not within +-2^21 or an origin_r or origin_r + d_r leaves [-2^20, 2^20].  The volume, the counts, the scores and
 *      the bests live in the CALLER's workspace (DEVICE, 256-byte aligned, svo_voxel_locate_workspace_bytes): nothing is allocated.
 *   d. One occupancy launch, one scores call, one copy of K*32 bytes to the host.
 *   e. Rank by descending hits_max, ties by ascending k; candidates with hits_max < min_hits are dropped.  None left:
 *      SVO_VOXEL_LOCATE_NO_CANDIDATE, pose7_out = pose7_in bit for bit (k = -1, rank = -1, coarse_pose7 = pose7_in, the rest 0).
 *   f. Each of the first n_refine ranked candidates: (u_k, T_r + (double)s_r * (double)voxel_size) through the align's step g to a
 *      pose7 (its coarse pose), then svo_voxel_map_align_plane if normals were given, else svo_voxel_map_align, with align_params.
 *   g. Eligible: refinements that ended CONVERGED or MAX_ITERS.  The largest last_matched wins, ties by the smallest last_cost, then
 *      by the earlier rank: SVO_VOXEL_LOCATE_FOUND, pose7_out the refined pose.  None eligible: SVO_VOXEL_LOCATE_UNREFINED, pose7_out
 *      the coarse pose of rank 0 and the result that of rank 0.
 *   Refusals, in this order: a null map; n < 0; n > 2^20; null pose7_in; null pose7_out; null result; null params; min_count < 1;
 *   up_axis outside 0..2; n_turn outside 0..31; turn_step not finite or outside (0, 0.25]; a box_r outside 0..16; the dims
 *   refusals of the occupancy; n_refine outside 1..63; min_hits < 1; the align's params refusals; null workspace; workspace not
 *   256-byte aligned; normals not 16-byte aligned; with n > 0 null points, then points not 4-byte aligned; then step c's.
 * The defaults are NOT tuned on real imagery.  Order of use: normals if wanted, then locate, then the cloud's own insert: locate
 * BEFORE inserting the cloud, as for the align.  The pipeline never locates by itself. */
typedef struct svo_voxel_locate_best {
  uint32_t hits_max;
  int32_t s0, s1, s2;
  uint32_t n_used, n_inside, index, zero;
} svo_voxel_locate_best; /* 32 bytes */
typedef struct svo_voxel_locate_params {
  int min_count;   /* >= 1: of the occupancy volume */
  int up_axis;     /* 0..2: the world axis the candidates turn about */
  int n_turn;      /* 0..31: K = 2 n_turn + 1 candidates */
  float turn_step; /* finite, in (0, 0.25]: b = j * turn_step / 2, the angle is 2 atan(b) */
  int box[3];      /* each 0..16: whole-voxel shifts |s_r| <= box_r */
  int dims[3];     /* the volume around the prior: each 1..2048, dims[0] a multiple of 64, product <= 2^30 */
  int n_refine;    /* 1..63: ranked candidates handed to the align */
  int min_hits;    /* >= 1: candidates whose peak is below this are dropped */
} svo_voxel_locate_params;
enum { SVO_VOXEL_LOCATE_FOUND = 0, SVO_VOXEL_LOCATE_UNREFINED = 1, SVO_VOXEL_LOCATE_NO_CANDIDATE = 2 };
#define SVO_VOXEL_LOCATE_MAX_K 63
#define SVO_VOXEL_LOCATE_MAX_BOX 16
typedef struct svo_voxel_locate_result {
  int status;        /* SVO_VOXEL_LOCATE_* */
  int k;             /* the chosen candidate */
  int shift[3];      /* its peak's shift, in voxels */
  uint32_t hits;     /* its peak */
  int rank;          /* its place in step e's order */
  int n_refined;     /* refinements run */
  double coarse_pose7[7];
  svo_voxel_align_result align; /* the chosen refinement's */
} svo_voxel_locate_result;
/* Bytes of a volume: d0*d1*d2/8.  Pure; SVO_ERR_INVALID and *bytes = 0 for dims the occupancy refuses. */
int svo_voxel_occupancy_bytes(const int* dims3, size_t* bytes);
/* Asynchronous on svo_stream(ctx): two memsets and one launch, one "voxel_occupancy" profile bracket. */
int svo_voxel_map_occupancy_dev(svo_voxel_map* map, int min_count, const int* origin3, const int* dims3, uint64_t* bits, uint32_t* counts);
/* svo_voxel_map_occupancy_dev into device memory of its own, copied to the HOST; synchronous; allocates and frees.  host_bits:
 * svo_voxel_occupancy_bytes bytes (any alignment); host_counts: 2 words, or NULL. */
int svo_voxel_map_occupancy(svo_voxel_map* map, int min_count, const int* origin3, const int* dims3, uint64_t* host_bits,
                            uint32_t* host_counts);
/* Asynchronous on svo_stream(ctx); one "voxel_locate" profile bracket. */
int svo_voxel_map_locate_scores_dev(svo_voxel_map* map, const uint64_t* bits, const int* origin3, const int* dims3,
                                    const svo_cloud_point* points, int n, const double* mats, int K, const int* box3, uint32_t* hits,
                                    svo_voxel_locate_best* best);
/* min_count 1, up_axis 1, n_turn 4, turn_step 0.04, box (8, 4, 8), dims (512, 128, 512) (4 MB), n_refine 3, min_hits 64.  NOT
 * tuned on real imagery.  Pure; SVO_ERR_INVALID for null params or a voxel_size that is not finite and > 0 (the voxel size is taken
 * for the day the defaults depend on it; today they do not). */
int svo_voxel_locate_default_params(float voxel_size, svo_voxel_locate_params* params);
/* Bytes of the loop's workspace: the volume, the counts, K*S0*S1*S2 scores and K bests, each part rounded up to 256 bytes.  Pure;
 * SVO_ERR_INVALID and *bytes = 0 for params the loop refuses. */
int svo_voxel_locate_workspace_bytes(const svo_voxel_locate_params* params, size_t* bytes);
/* The host loop above, synchronous.  normals: the DEVICE array of svo_voxel_map_normals_dev (plane form of the refinement), or NULL
 * (point form).  pose7_in, pose7_out (may be the same array) and result on the HOST. */
int svo_voxel_map_locate(svo_voxel_map* map, const svo_voxel_normal* normals, const svo_cloud_point* points, int n,
                         const double* pose7_in, const svo_voxel_locate_params* params, const svo_voxel_align_params* align_params,
                         void* workspace, double* pose7_out, svo_voxel_locate_result* result);

/* Voxel map sight lines: what a straight line through the occupancy volume meets first.  A ray walk through the dense
 * bit volume of svo_voxel_map_occupancy_dev: a hole-free depth view in the dense track's CV_16S format, visibility and
 * segment-collision queries for arbitrary rays, and the 3D sight lines a view planner needs.  Integer work apart from a few
 * ordered f64 operations per ray (no contraction); a restatement in another language gives the same bytes.
 * Inputs bits, origin3, dims3 are exactly those of svo_voxel_map_occupancy_dev, with the same refusals in the same order.  The map
 * argument is read for voxel_size and the stream ONLY.  The table is not touched.
 *
 * 1. Coarse volume (svo_voxel_occupancy_coarse_dev).  cd_r = (d_r + 7) >> 3.  Coarse bit Bc = b0 + cd0*(b1 + cd1*b2) lives in
 *    little-endian u64 words, (cd0*cd1*cd2 + 63) >> 6 of them.  A coarse bit is 1 iff any fine bit with j_r >> 3 == b_r is 1.  Bits
 *    past the last block are 0.  svo_voxel_occupancy_coarse_bytes(dims3, &bytes) is pure.  The entry issues one memset and one
 *    launch, under profile tag "voxel_coarse".  coarse is a DEVICE pointer, 8-byte aligned.  Refusals, in this order: a null map;
 *    the dims refusals of the occupancy; null bits; bits not 8-byte aligned; null coarse; coarse not 8-byte aligned.
 *
 * 2. A ray is the 32-byte record svo_voxel_ray {float ox, oy, oz, max_range, dx, dy, dz; uint32_t tag}.  Rays are 16-byte aligned,
 *    in world metres.  d may have any length.  tag is carried and never read.  Set-up is in doubles, each f32 widened first, in
 *    the written order:
 *      REJECTED iff any of the seven floats is not finite, or max_range < 0, or m = max(|dx|, |dy|, |dz|) == 0.
 *      REJECTED also iff any q_r = o_r / (double)voxel_size fails q_r >= -1048560.0 && q_r < 1048560.0.
 *      p_r = (int64)floor(q_r * 256.0) - 256*origin_r.  This is the position in 1/256 voxel, relative to the volume.
 *      D_r = (int)floor((d_r / m) * 16384.0 + 0.5).  The largest component is exactly +-16384.
 *      S = D_0^2 + D_1^2 + D_2^2.
 *      R = (max_range / (double)voxel_size) * 256.0.
 *      L_r = (int64)min(floor((R * (double)|D_r|) / sqrt((double)S)), 2^40), the min taken in f64.
 *
 * 3. The walk.  The rule is stated for one ray.  Every implementation must return exactly these values.
 *    Start: c_r = p_r >> 8 (arithmetic shift) and f_r = p_r & 255.  OUTSIDE iff some c_r is not in [0, d_r).  There is no walk and
 *    no entry into the volume from outside: the volume is meant to be centred on the viewer.  Step count k = 0.  A visited cell is
 *    TESTED iff k >= min_step (min_step in 0..255).  It is a HIT iff tested and its bit is 1.  The start cell is visited at k = 0
 *    (HIT there: axis = 3, n = 0).
 *    Per-axis state: n_r = 256 - f_r if D_r > 0, f_r if D_r < 0.  w_r is the product of max(|D_s|, 1) over the other two axes.
 *    X_r = n_r*w_r, or 2^62 if D_r == 0.
 *    Repeat:
 *      1. a = the axis with the smallest X, ties to the smallest axis number.
 *      2. If n_a > L_a: RANGE.  Stop.
 *      3. c_a += sign(D_a).  If that leaves [0, d_a): LEFT.  Stop.
 *      4. k += 1.  Visit the cell.  HIT: stop.
 *      5. n_a += 256, X_a += 256*w_a.
 *    Bounds and loop length: X < 2^48, so every compare is a 64-bit integer compare and every update an add.  The loop makes at
 *    most d0 + d1 + d2 steps by construction.  The kernel also carries that number as an explicit iteration cap, so that no input
 *    can make a wavefront spin.
 *
 * 4. Result is the 16-byte record svo_voxel_ray_hit {uint32_t cell, steps; float dist; uint32_t status}.  status = code | axis << 8.
 *    Codes: HIT 0, LEFT 1, RANGE 2, OUTSIDE 3, REJECTED 4.  axis is the a of the last crossing considered, or 3 where there was
 *    none.  cell is the bit number B of the last cell visited.  It is 0xFFFFFFFF for OUTSIDE and REJECTED.  steps = k.
 *    dist = (float)((((double)n_a * sqrt((double)S)) / (double)|D_a|) / 256.0 * (double)voxel_size), with the n_a of that last
 *    crossing.  It is 0.0f where there was none.
 *
 * 5. Counts.  counts = 6 DEVICE u64 (or NULL): {n_hit, n_left, n_range, n_outside, n_rejected, n_steps = sum of steps}.  They are
 *    zeroed on the stream.  One relaxed atomicAdd is issued per workgroup and non-zero counter.  There is no fence and no waiting
 *    on another workgroup.
 *
 * 6. svo_voxel_occupancy_rays_dev(map, bits, coarse_or_NULL, origin3, dims3, rays, n, min_step, hits, counts).  n <= 2^20.  hits
 *    holds n records, 16-byte aligned.  Every record is written by every call.  n == 0 launches nothing but the counts' memset.
 *    coarse == NULL selects the plain walk.  A given coarse selects the block-skipping walk: while the current cell's coarse bit
 *    is 0, all crossings up to the one that leaves the cell's 8-block (or the volume through it) are made at once, if none of
 *    them breaks n <= L (host/voxel_rays.h).  The two walks give the same bytes.  coarse is trusted to be item 1's
 *    output for these bits.  Profile tag "voxel_rays".
 *    Refusals, in this order, each with nothing launched: null map; n < 0; n > 2^20; min_step outside 0..255; the origin and dims
 *    refusals of the occupancy; null bits, then bits misaligned; coarse misaligned; null hits, then hits misaligned; counts not
 *    8-byte aligned; with n > 0: null rays, then rays misaligned.
 *
 * 7. svo_voxel_occupancy_rays is the synchronous host form: HOST rays in, HOST hits and counts out (counts may be NULL; no
 *    alignment is asked of the host arrays).  It allocates and frees its own device copies of rays, hits and counts.  bits and
 *    coarse stay DEVICE pointers.
 *
 * 8. Camera form (svo_voxel_occupancy_raycast_dev, _raycast_pose7_dev).  Inputs are width, height, cam (focal, cx, cy, baseline
 *    read), c2w12 (CAMERA->WORLD, 12 HOST doubles by value; the pose7 form goes through svo_pose7_to_cam_to_world), and
 *    svo_voxel_raycast_params {float max_range; int min_step;}.  The defaults are 30.0 and 1.  There is one ray per pixel (x, y):
 *      v0 = ((double)x - cx) / focal, v1 = ((double)y - cy) / focal.
 *      d_r = m[r][0]*v0 + m[r][1]*v1 + m[r][2], left to right.  o_r = m[r][3].
 *      Item 2's set-up is applied to these doubles (nothing is narrowed to f32), then item 3's walk.
 *    The output is disp16, a tight CV_16S map in sixteenths.  A HIT with k >= 1 gives
 *      z = ((double)n_a * (double)voxel_size * 64.0) / ((double)|D_a| * m).
 *    This is the depth along the optical axis of the point where the ray enters the hit voxel.
 *      d16 = floor((focal*baseline) / z * 16.0 + 0.5).  It is kept iff 1.0 <= d16 && d16 <= 32767.0, compared in f64.
 *    Every other pixel is FILTERED (-16).  cell is a tight u32 per pixel, or NULL.  It is 0xFFFFFFFF where disp16 is FILTERED.
 *    counts is as in item 5 plus a seventh word, n_pixels, the kept pixels.  A wavefront takes an 8 x 8 pixel tile.
 *    Refusals, in this order: null map; null cam; null c2w12 (pose7 form: null pose7); null params; max_range not finite or < 0;
 *    min_step outside 0..255; width or height < 1 or beyond the context's limits; focal or baseline not finite or <= 0; then
 *    item 6's refusals for the volume (origin, dims, bits, coarse); null disp16; disp16 not 2-byte aligned; cell not 4-byte
 *    aligned; counts not 8-byte aligned.
 *
 * 9. Host convenience svo_voxel_map_raycast.  It takes map, min_count, dims3, width, height, cam, c2w12, params, and HOST outputs.
 *    The volume's origin comes from the camera centre (m[r][3]) by the locate's step c.  The call then runs occupancy, coarse and
 *    raycast, and copies out.  It is synchronous, and allocates and frees.  Refusals: null map; min_count < 1; item 8's for cam, c2w12, params, width and height; the dims refusals; null disp16;
 *    then step c's.
 * The defaults are NOT tuned on real imagery.  Order of use: occupancy after the map's last insert / update / carve, then coarse,
 * then rays.  The pipeline never casts rays by itself. */
typedef struct svo_voxel_ray {
  float ox, oy, oz, max_range;
  float dx, dy, dz;
  uint32_t tag;
} svo_voxel_ray; /* 32 bytes */
typedef struct svo_voxel_ray_hit {
  uint32_t cell, steps;
  float dist;
  uint32_t status;
} svo_voxel_ray_hit; /* 16 bytes */
enum { SVO_VOXEL_RAY_HIT = 0, SVO_VOXEL_RAY_LEFT = 1, SVO_VOXEL_RAY_RANGE = 2, SVO_VOXEL_RAY_OUTSIDE = 3, SVO_VOXEL_RAY_REJECTED = 4 };
typedef struct svo_voxel_raycast_params {
  float max_range; /* finite, >= 0: metres along the ray */
  int min_step;    /* 0..255: cells visited before this step are not tested (1: the viewer's own cell is skipped) */
} svo_voxel_raycast_params;
/* max_range 30.0, min_step 1.  NOT tuned on real imagery.  Pure. */
int svo_voxel_raycast_default_params(svo_voxel_raycast_params* params);
/* Bytes of a coarse volume.  Pure; SVO_ERR_INVALID and *bytes = 0 for dims the occupancy refuses. */
int svo_voxel_occupancy_coarse_bytes(const int* dims3, size_t* bytes);
/* Asynchronous on svo_stream(ctx): one memset and one launch, one "voxel_coarse" profile bracket. */
int svo_voxel_occupancy_coarse_dev(svo_voxel_map* map, const uint64_t* bits, const int* dims3, uint64_t* coarse);
/* Asynchronous on svo_stream(ctx): the counts' memset and one launch, one "voxel_rays" profile bracket. */
int svo_voxel_occupancy_rays_dev(svo_voxel_map* map, const uint64_t* bits, const uint64_t* coarse, const int* origin3, const int* dims3,
                                 const svo_voxel_ray* rays, int n, int min_step, svo_voxel_ray_hit* hits, uint64_t* counts);
/* Item 7: HOST rays, hits and counts (6 words, or NULL); bits and coarse on the DEVICE.  Synchronous; allocates and frees. */
int svo_voxel_occupancy_rays(svo_voxel_map* map, const uint64_t* bits, const uint64_t* coarse, const int* origin3, const int* dims3,
                             const svo_voxel_ray* host_rays, int n, int min_step, svo_voxel_ray_hit* host_hits, uint64_t* host_counts);
/* Item 8.  DEVICE pointers; cell and counts (7 words) may be NULL.  Asynchronous; one "voxel_rays" profile bracket. */
int svo_voxel_occupancy_raycast_dev(svo_voxel_map* map, const uint64_t* bits, const uint64_t* coarse, const int* origin3, const int* dims3,
                                    int width, int height, const svo_camera_info* cam, const double* c2w12,
                                    const svo_voxel_raycast_params* params, int16_t* disp16, uint32_t* cell, uint64_t* counts);
/* svo_pose7_to_cam_to_world, then svo_voxel_occupancy_raycast_dev. */
int svo_voxel_occupancy_raycast_pose7_dev(svo_voxel_map* map, const uint64_t* bits, const uint64_t* coarse, const int* origin3,
                                          const int* dims3, int width, int height, const svo_camera_info* cam, const double* pose7,
                                          const svo_voxel_raycast_params* params, int16_t* disp16, uint32_t* cell, uint64_t* counts);
/* Item 9.  HOST outputs: disp16 width*height int16; cell width*height u32 or NULL; counts 7 u64 or NULL; origin3_out: the volume's
 * origin, 3 ints, or NULL. */
int svo_voxel_map_raycast(svo_voxel_map* map, int min_count, const int* dims3, int width, int height, const svo_camera_info* cam,
                          const double* c2w12, const svo_voxel_raycast_params* params, int16_t* disp16, uint32_t* cell, uint64_t* counts,
                          int* origin3_out);

/* Voxel map distance field: how far every voxel of the occupancy volume is from the nearest occupied one.  The exact
 * squared Euclidean distance in voxels, the nearest occupied cell, the distance in map units, the volume inflated by a radius (in
 * the occupancy's own bit format, so that svo_voxel_occupancy_rays_dev over it is a swept-sphere test) and a per-point query.
 * Integers only but for rule 5 and a sphere's set-up; nothing depends on thread order; a restatement in another language gives
 * the same bytes.  Inputs bits, dims3 and (the query, the host call) origin3 are exactly those of svo_voxel_map_occupancy_dev, with
 * the same refusals in the same order.  Bit number B = j0 + d0*(j1 + d1*j2).  The map argument is read for voxel_size and the stream
 * ONLY.  The table is not touched.
 *   svo_voxel_distance_params {int max_dist; float inflate_radius;}: max_dist in voxels, 1..254; inflate_radius in map units, finite
 *   and >= 0.  The defaults are 32 and 0, NOT tuned on real data.
 * 1. A cell is a source iff its bit is 1.  Cells outside the volume are never sources.  Axis 0 does not run on from the end of one
 *    row into the next row.
 * 2. dist2[B] (u16, required) is the minimum over sources s of sum_r (j_r - s_r)^2 if that is <= max_dist^2, else NONE16 = 0xFFFF.
 *    A source has 0.  254^2 = 64,516 fits.
 * 3. nearest[B] (u32, optional) is the smallest bit number among the sources that attain the minimum, 0xFFFFFFFF where dist2 is
 *    NONE16.
 * 4. inflated (u64 words in the occupancy's layout, svo_voxel_occupancy_bytes of them, optional): bit B is 1 iff dist2[B] <= R2, with
 *    rc = (double)inflate_radius / (double)voxel_size and R2 = floor(rc*rc) clamped to max_dist^2, computed once on the host (an
 *    overflowing quotient or square takes the clamp).  Sources are therefore always set.  Every word is written by every call: no
 *    memset is needed.
 * 5. clearance[B] (f32, optional) = (float)(sqrt((double)dist2) * (double)voxel_size), +infinity where dist2 is NONE16.
 * 6. counts = 4 DEVICE u64 {n_sources, n_reached (0 < dist2 <= max_dist^2), n_unreached (NONE16), n_inflated (the set bits of rule
 *    4's volume, sources included, counted whether or not inflated is given)}, or NULL.  Zeroed on the stream; one relaxed
 *    atomicAdd per workgroup and non-zero counter.  No fence, no waiting on another workgroup.
 * 7. The workspace is the caller's: svo_voxel_distance_workspace_bytes(dims3, want_nearest, &bytes) DEVICE bytes, 8-byte aligned, 3
 *    per cell without nearest and 6 with it (want_nearest must be non-zero iff out->nearest is given).  Its contents are free on
 *    entry and meaningless afterwards.
 * 8. svo_voxel_occupancy_distance_dev refuses, in this order, each with SVO_ERR_INVALID, the argument named and nothing launched:
 *    null map; null params; max_dist outside 1..254; inflate_radius not finite or negative; the dims refusals of the occupancy;
 *    null bits, then bits misaligned; null workspace, then workspace not 8-byte aligned; null out; null dist2; dist2 not 2-byte
 *    aligned; nearest, then clearance not 4-byte aligned; inflated not 8-byte aligned; counts not 8-byte aligned.
 * 9. Query (svo_voxel_distance_query_dev).  A sphere is the 16-byte record svo_voxel_sphere {float x, y, z, radius} in world metres,
 *    a result the 16-byte record svo_voxel_sphere_hit {uint32_t cell, dist2; float clearance; uint32_t code}.  In doubles, each f32
 *    widened first: q_r = x_r / (double)voxel_size.  REJECTED (3) unless radius >= 0 and finite and every q_r >= -1048560.0 &&
 *    q_r < 1048560.0 (a NaN and the infinities fail).  j_r = (int)floor(q_r) - origin_r.  OUTSIDE (2) iff some j_r is not in [0, d_r).
 *    For both, cell and dist2 are 0xFFFFFFFF and clearance is +infinity.  Otherwise cell = B, dist2 is dist2[B] widened (NONE16
 *    becomes 0xFFFFFFFF), clearance follows rule 5, and the code is COLLIDES (1) iff (double)dist2 <= floor(rc*rc) with
 *    rc = (double)radius / (double)voxel_size, per sphere and without a clamp, else FREE (0).  A cell beyond max_dist therefore
 *    collides only with a radius of 65,536 voxels or more.  This is cell centre to cell centre; a caller who wants a
 *    conservative test adds sqrt(3) * voxel_size to the radius.  counts = 6 DEVICE u64 {n, n_free, n_collides, n_outside,
 *    n_rejected, n_beyond (inside the volume, dist2 NONE16)}, or NULL.  n <= 2^20; n == 0 launches nothing but the counts' memset.
 *    Profile tag "voxel_distance_query".  Refusals, in this order: null map; n < 0; n > 2^20; the origin and dims refusals of the
 *    occupancy; null dist2, then dist2 not 2-byte aligned; null hits, then hits not 16-byte aligned; counts not 8-byte aligned; with
 *    n > 0: null spheres, then spheres not 16-byte aligned.
 * 10. svo_voxel_distance_query is the synchronous host form: HOST spheres in, HOST hits and counts out (counts may be NULL; no
 *    alignment is asked of the host arrays); dist2 stays a DEVICE pointer.  It allocates and frees.
 * 11. svo_voxel_map_distance runs svo_voxel_map_occupancy_dev and the distance field into device memory of its own and copies the
 *    asked outputs to the HOST; synchronous; allocates and frees.  Refusals: null map; min_count < 1; the params refusals of rule 8;
 *    the origin and dims refusals; null out; null dist2.
 * Order of use: occupancy after the map's last insert / update / carve, then distance, then queries, or rays over inflated.  The
 * pipeline never calls any of this by itself. */
typedef struct svo_voxel_distance_params {
  int max_dist;         /* 1..254 voxels: farther sources are not looked for */
  float inflate_radius; /* finite, >= 0, map units: rule 4 */
} svo_voxel_distance_params;
typedef struct svo_voxel_distance_out {
  uint16_t* dist2;    /* required */
  uint32_t* nearest;  /* or NULL */
  float* clearance;   /* or NULL */
  uint64_t* inflated; /* or NULL */
} svo_voxel_distance_out;
typedef struct svo_voxel_sphere {
  float x, y, z, radius;
} svo_voxel_sphere; /* 16 bytes */
typedef struct svo_voxel_sphere_hit {
  uint32_t cell, dist2;
  float clearance;
  uint32_t code;
} svo_voxel_sphere_hit; /* 16 bytes */
enum { SVO_VOXEL_SPHERE_FREE = 0, SVO_VOXEL_SPHERE_COLLIDES = 1, SVO_VOXEL_SPHERE_OUTSIDE = 2, SVO_VOXEL_SPHERE_REJECTED = 3 };
/* max_dist 32, inflate_radius 0.  NOT tuned on real data.  Pure; SVO_ERR_INVALID for null out or a voxel_size that is not finite and
 * > 0 (the voxel size is taken for the day the defaults depend on it; today they do not). */
int svo_voxel_distance_default_params(float voxel_size, svo_voxel_distance_params* out);
/* Rule 7.  Pure; SVO_ERR_INVALID and *bytes = 0 for dims the occupancy refuses. */
int svo_voxel_distance_workspace_bytes(const int* dims3, int want_nearest, size_t* bytes);
/* Bytes of dist2: 2 per cell.  Pure; SVO_ERR_INVALID and *bytes = 0 for dims the occupancy refuses. */
int svo_voxel_distance_bytes(const int* dims3, size_t* bytes);
/* Asynchronous on svo_stream(ctx): the counts' memset and three launches, one "voxel_distance" profile bracket.  DEVICE pointers. */
int svo_voxel_occupancy_distance_dev(svo_voxel_map* map, const uint64_t* bits, const int* dims3, const svo_voxel_distance_params* params,
                                     void* workspace, const svo_voxel_distance_out* out, uint64_t* counts);
/* Rule 9.  DEVICE pointers.  Asynchronous; one "voxel_distance_query" profile bracket. */
int svo_voxel_distance_query_dev(svo_voxel_map* map, const uint16_t* dist2, const int* origin3, const int* dims3,
                                 const svo_voxel_sphere* spheres, int n, svo_voxel_sphere_hit* hits, uint64_t* counts);
/* Rule 10: HOST spheres, hits and counts (6 words, or NULL); dist2 on the DEVICE.  Synchronous; allocates and frees. */
int svo_voxel_distance_query(svo_voxel_map* map, const uint16_t* dist2, const int* origin3, const int* dims3,
                             const svo_voxel_sphere* host_spheres, int n, svo_voxel_sphere_hit* host_hits, uint64_t* host_counts);
/* Rule 11.  host_out: HOST arrays (dist2 required, any alignment; inflated holds svo_voxel_occupancy_bytes bytes); host_counts: 4
 * u64, or NULL. */
int svo_voxel_map_distance(svo_voxel_map* map, int min_count, const int* origin3, const int* dims3,
                           const svo_voxel_distance_params* params, const svo_voxel_distance_out* host_out, uint64_t* host_counts);

/* Voxel map route: from every cell of the occupancy volume the cost of the cheapest way through free space to a goal cell, the first
 * move of that way, and the cells of the way from given start cells: what a planner asks a volumetric map second, and
 * what anything that leaves the ground plane - a drone, an arm, a vehicle on a ramp under a bridge - cannot ask the ground plan.  The
 * ground plan route lifted to 26 neighbours.  Integers only; a converged result is the unique fixed point of the relaxation,
 * depends on no thread order and is tested with ==.  The map argument is read for the stream ONLY.  The table is not touched.
 * INPUTS (device memory for the _dev entry): closed, u64 words in the occupancy's layout (svo_voxel_occupancy_bytes of them),
 * required: cell B = j0 + d0*(j1 + d1*j2) is passable iff bit B is 0 (the distance field's inflated fits as it is, and so do the
 * occupancy bits themselves); dims3, with the occupancy's checks, messages and order; dist2, u16 per cell or NULL (the distance
 * field's array, 0xFFFF meaning far); goals, n_goals (1..65536) u32 cell numbers; starts, n_starts (0..4096) u32 cell numbers, NULL
 * iff n_starts == 0.
 *   1. pen[v] = near_weight * (near_r2 - dist2[v]) where dist2 is given and dist2[v] < near_r2, else 0 (0xFFFF is far, a NULL dist2
 *      is far everywhere).
 *   2. The 26 neighbours are coded k = 9*(dj2+1) + 3*(dj1+1) + (dj0+1), 0..26 without 13.  A move from v to u is allowed iff both
 *      cells are inside the volume and passable and every other cell of the box spanned by v and u is passable: 2 cells for an
 *      edge move (two coordinates change), 6 for a vertex move (three change) - the ground plan route's no-corner-cutting rule in
 *      3D.  Axis 0 never runs on from the end of one row into the next.  The move costs w * (16 + pen[u]), w = 5 / 7 / 9 for 1 / 2
 *      / 3 changed coordinates: the penalty of the cell entered.  One step stays below 2^24.  With these weights a one-layer
 *      volume (d2 = 1) has exactly the ground plan route's 5-7 field.
 *   3. A goal >= d0*d1*d2 or on a closed cell is ignored; the others have cost 0.
 *   4. cost[B] (u32, required) is the cheapest sum of move costs from B to any used goal if that sum is <= max_cost, else
 *      SVO_VOXEL_ROUTE_NONE = 0xFFFFFFFF; closed cells are NONE.  Every prefix of a route within the cap is within the cap, so the
 *      capped field is the true one truncated; candidates never exceed 0x7F000000 + 2^24, so u32 arithmetic does not wrap.
 *   5. next[B] (u8, optional) is 13 at a used goal, otherwise the smallest k whose move is allowed and has cost[u_k] + step ==
 *      cost[B], and 255 where cost is NONE.  Following next strictly lowers cost, so it ends at a goal.
 *   6. Paths (optional, all three or none): path n_starts x max_path u32, path_len n_starts u32, path_status n_starts u8.  Row i holds
 *      the cells from starts[i] along next to the goal, both ends included; path_len[i] is the full number of cells, only the first
 *      max_path are written and row entries past the written ones are not touched.  Status SVO_VOXEL_ROUTE_OK, _TRUNCATED (len >
 *      max_path), _UNREACHED (cost NONE; len 0), _OUT_OF_VOLUME (len 0) or _NOT_CONVERGED (len 0).
 *   7. counts: 8 u64 on the device, or NULL: {n_goals_used, n_reached, n_unreached, n_closed, converged, rounds_run, 0, 0}.  They
 *      are zeroed on the stream.  n_reached counts passable cells with a cost, goals included; n_reached + n_unreached + n_closed
 *      = d0*d1*d2; n_goals_used counts list entries, so a duplicate counts twice.
 *   8. The call enqueues max_rounds relaxation rounds.  converged is 1 iff a further round would have nothing to do.  If it is 0,
 *      cost holds upper bounds whose bits may depend on timing, next and path are not written, every path_len is 0 and every status
 *      _NOT_CONVERGED, and the three cell counts stay 0.  rounds_run (the last round of this call in which a tile had work) is
 *      reported but may depend on how workgroups interleave.  A call with resume = 1, the same closed, dims3, dist2, goals and
 *      params and the same workspace and cost buffers untouched since, continues where the earlier call stopped; repeating such
 *      calls reaches converged = 1 and the unique field.
 *   9. workspace: svo_voxel_route_workspace_bytes(dims3, &bytes) bytes of device memory, 8-byte aligned, contents free on entry
 *      unless resume: a header, two activity words per tile and one direction byte per cell.  closed, dist2, goals and starts are
 *      only read and must not overlap an output.
 *  10. svo_voxel_occupancy_route_dev refuses, in this order, each with SVO_ERR_INVALID, the argument named, nothing launched and the
 *      context still usable: null map; null params; near_r2 > 254^2; near_weight * near_r2 > 2^20; max_cost outside 1..0x7F000000;
 *      max_rounds outside 1..4096; max_path outside 1..2^20 (only when n_starts > 0); resume not 0 or 1; the dims refusals of the
 *      occupancy; null closed, then closed not 8-byte aligned; null goals; n_goals outside 1..65536; n_starts outside 0..4096;
 *      starts NULL with n_starts > 0, then non-NULL with n_starts == 0; null workspace; null out; null cost; any of path, path_len,
 *      path_status NULL while another is not, then non-NULL with n_starts == 0; cost, goals, starts, path, path_len off 4 bytes;
 *      dist2 off 2 bytes; workspace, then counts off 8 bytes.
 * UNIQUENESS.  With positive integer step costs the equations cost[goal] = 0, cost[v] = min over allowed moves of cost[u] + step have
 * one solution, the shortest-route cost; relaxation only lowers a word towards it and never below, in whatever order cells are
 * relaxed.  That is what lets the tiled parallel form be compared with == against Dijkstra.
 * The defaults are NOT tuned on real data: near_r2 0, near_weight 0, max_cost 0x7F000000, max_rounds 32, max_path 4096, resume 0.
 * 32 rounds cover random clutter and open space in a volume of 128 x 32 x 128 (the CPU trial of DESIGN 7v); a larger volume, a goal
 * far from the volume's centre or a maze of slabs takes more rounds or resume.
 * Order of use: occupancy, then distance (for inflated and dist2), then the route.  The pipeline never computes a route by itself
 * (INTEGRATION 4a). */
#define SVO_VOXEL_ROUTE_NONE 0xFFFFFFFFu
#define SVO_VOXEL_ROUTE_MAX_COST 0x7F000000u
enum { SVO_VOXEL_ROUTE_OK = 0, SVO_VOXEL_ROUTE_TRUNCATED = 1, SVO_VOXEL_ROUTE_UNREACHED = 2, SVO_VOXEL_ROUTE_OUT_OF_VOLUME = 3,
       SVO_VOXEL_ROUTE_NOT_CONVERGED = 4 };
typedef struct svo_voxel_route_params {
  uint32_t near_r2;     /* 0..254^2: squared radius, in voxels, inside which the penalty applies */
  uint32_t near_weight; /* near_weight * near_r2 <= 2^20: penalty per unit of near_r2 - dist2 */
  uint32_t max_cost;    /* 1..0x7F000000: cap on a cell's cost */
  int max_rounds;       /* 1..4096: relaxation rounds this call enqueues */
  int max_path;         /* 1..2^20, read only when n_starts > 0: cells written per path */
  int resume;           /* 0 or 1: continue an earlier call's field */
} svo_voxel_route_params;
typedef struct svo_voxel_route_out { /* every pointer but cost may be NULL; path, path_len and path_status only together */
  uint32_t* cost;       /* d0*d1*d2 */
  uint8_t* next;        /* d0*d1*d2 */
  uint32_t* path;       /* n_starts * max_path */
  uint32_t* path_len;   /* n_starts */
  uint8_t* path_status; /* n_starts */
} svo_voxel_route_out;
/* The defaults above.  Pure; SVO_ERR_INVALID for null out or a voxel_size that is not finite and > 0 (the voxel size is taken for
 * the day the defaults depend on it; today they do not). */
int svo_voxel_route_default_params(float voxel_size, svo_voxel_route_params* out);
/* Rule 9.  Pure; SVO_ERR_INVALID and *bytes = 0 for dims the occupancy refuses. */
int svo_voxel_route_workspace_bytes(const int* dims3, size_t* bytes);
/* The cell number B of the world position xyz3 (three floats, map units) in the volume of origin3 and dims3, by exactly the distance
 * field's rule 9: what goals and starts are formed with.  Pure; SVO_ERR_INVALID for a null pointer, a voxel_size that is not finite
 * and > 0, an origin or dims the occupancy refuses, and a rejected or outside position. */
int svo_voxel_occupancy_cell_of(float voxel_size, const int* origin3, const int* dims3, const float* xyz3, uint32_t* cell);
/* DEVICE pointers, asynchronous on the map's stream.  Everything it enqueues is one "voxel_route" profile bracket. */
int svo_voxel_occupancy_route_dev(svo_voxel_map* map, const uint64_t* closed, const int* dims3, const uint16_t* dist2,
                                  const svo_voxel_route_params* params, const uint32_t* goals, int n_goals, const uint32_t* starts,
                                  int n_starts, void* workspace, const svo_voxel_route_out* out, uint64_t* counts);
/* closed and dist2 stay DEVICE pointers; goals, starts, the outputs and counts (8 u64 or NULL) are HOST arrays of any alignment.
 * Synchronous: one device allocation for the call, freed after the stream is drained whatever failed.  The refusals of rule 10
 * without the workspace's and the host arrays' alignments; resume = 1 is refused after the params' ranges: the workspace does not
 * outlive the call. */
int svo_voxel_occupancy_route(svo_voxel_map* map, const uint64_t* closed, const int* dims3, const uint16_t* dist2,
                              const svo_voxel_route_params* params, const uint32_t* goals, int n_goals, const uint32_t* starts,
                              int n_starts, const svo_voxel_route_out* out, uint64_t* counts);

/* Voxel map grid: the ground plan of the map, an axis-aligned na x nb grid over two of the map's axes.  Per cell: the highest and
 * the lowest surface inside a height band, the mean intensity of the highest voxel, how many voxels and points fell into the cell,
 * and a class (UNKNOWN, LEVEL, OBSTACLE).  One walk over the table bins every qualifying voxel by its KEY, in integers only; a second
 * launch turns the cells into the outputs.  The grid is tested with ==.
 *   Axes.  up_axis (0..2) is the map axis that points up or down, up_sign (+1 / -1) says which: a world frame that is the first
 *      camera's frame has y down, i.e. up_axis 1, up_sign -1.  The grid's axes are the other two in cyclic order, a = (up_axis+1) % 3,
 *      b = (up_axis+2) % 3: for the camera convention z forward and x right.  Cell (ia, ib) is element ia*nb + ib of every output.
 *   Host-side conversion, once per call, with vs = (double)voxel_size, stated f64 operations:
 *      ka0 = floor(origin_a / vs), kb0 = floor(origin_b / vs), each clamped to +-2^21;
 *      hlo = floor(up_lo / vs * 65536.0), hhi = floor(up_hi / vs * 65536.0) (divide, then multiply), each clamped to +-2^38, as int64;
 *      step = floor(obstacle_step / vs * 65536.0), clamped to 0..2^38.
 *   Per slot, integers only:
 *   1. A slot qualifies iff key != EMPTY and count = ci >> 40 >= min_count (>= 1).  Carved slots have count 0 and never qualify;
 *      nothing divides by 0.
 *   2. g = k_up * 65536 + s_up div count: k_up the signed key index of the up axis (its 21 key bits minus 2^20), s_up that axis's
 *      sum word, div the exact integer floor division.  The quotient is at most 65535 because every fraction is, so g is the
 *      voxel's mean height in 65536ths of a voxel.  hgt = up_sign * g, |hgt| < 2^37.
 *   3. In the band iff hlo <= hgt && hgt <= hhi.
 *   4. ia = floordiv(k_a - ka0, cell_voxels), ib = floordiv(k_b - kb0, cell_voxels): the FLOOR, not truncation (the voxel at
 *      k_a - ka0 = -1 is outside, not in cell 0).  Binned iff 0 <= ia < na && 0 <= ib < nb; cell = ia*nb + ib.
 *   5. Four u64 words per cell, in the caller's workspace at 4*cell .. 4*cell + 3:
 *        top  = max(top, (uint64)(hgt + 2^37) << 8 | isum div count)      (isum: the low 40 bits of ci)
 *        bot  = max(bot, (uint64)(2^37 - hgt))
 *        nvox += 1
 *        npts += count
 *      by relaxed device-scope 64-bit atomics whose value is not read back.  max and + commute: the grid depends on no thread
 *      order and on no slot placement.  Among voxels of equal height the larger mean intensity wins the cell.  Both max words are
 *      never 0 for a binned voxel.
 *   6. Resolve, a second launch on the same stream, per cell.  nvox == 0: cls = 0 (SVO_VOXEL_GRID_UNKNOWN), top = -infinity,
 *      bottom = +infinity, intensity = 0, n_voxels = 0, n_points = 0.  Otherwise htop = (top >> 8) - 2^37, hbot = 2^37 - bot,
 *      cls = htop - hbot > step ? 2 (SVO_VOXEL_GRID_OBSTACLE) : 1 (SVO_VOXEL_GRID_LEVEL),
 *      top = (float)((double)htop / 65536.0 * vs) and bottom likewise from hbot (heights in map units along UP, whatever up_sign),
 *      intensity = top word & 255, n_voxels = nvox (u32: a table has at most 2^28 slots), n_points = npts (u64, nothing saturates).
 *   7. counts = {n_qualifying, n_in_band, n_binned, n_cells, n_obstacle}: 5 u64 on the device, or NULL.  n_cells: cells with
 *      nvox > 0; n_obstacle: cells of class 2; the resolve counts these two.  One relaxed atomicAdd per workgroup and non-zero
 *      counter.
 *   8. SVO_ERR_INVALID with the argument named, and nothing launched, for: a null map, params, workspace, out or out->cls; up_axis
 *      outside 0..2; up_sign other than +1 and -1; an origin that is not finite; cell_voxels outside 1..1024; na or nb outside
 *      1..8192 or na*nb > 2^24; a NaN up_lo or up_hi (infinities are allowed) or up_lo > up_hi; obstacle_step negative or NaN;
 *      min_count < 1; a workspace or counts that is not 8-byte aligned; top, bottom or n_voxels not 4-byte, n_points not 8-byte
 *      aligned.
 * workspace: svo_voxel_grid_workspace_bytes(na, nb) = 32*na*nb bytes of device memory, 8-byte aligned; its contents before the
 * call are meaningless (it is zeroed on the stream before the first launch), afterwards it holds the four words of every cell.
 * A table that only inserts ever wrote holds quotients <= 65535 (heights) and <= 255 (intensities).  The removal's KNOWN PROPERTY
 * (item 6 of "Voxel map removal") can leave larger ones; both divisions are exact for every sum below 2^40 and count below 2^24,
 * and the words are formed as written above in 64-bit arithmetic.
 * KNOWN PROPERTIES.  The grid is aligned with the map's axes and is not rotated: a first camera that was pitched gives a tilted
 * "up".  A cell's class is only the span between its highest and lowest voxel inside the band: a slope steeper than
 * obstacle_step per cell is an obstacle, an overhang above the band is not seen.  What lies BETWEEN cells (a kerb on a cell
 * boundary, a long gentle slope, a cell alone in unknown ground) is "Ground plan surface"'s, below.
 * The defaults are NOT tuned on real imagery: the camera convention (up_axis 1, up_sign -1), cells of 0.5 map units (cell_voxels =
 * floor(0.5 / vs + 0.5) clamped to 1..1024, 5 at the default voxel size), 256 x 256 cells starting at a = 0 and centred on b = 0
 * (origin_a = 0, origin_b = -128 * cell_voxels * vs), the band -3 .. +2.5, obstacle_step 0.3, min_count 1.
 * The pipeline never builds a grid by itself; call it after the ledger's updates and the carve. */
#define SVO_VOXEL_GRID_UNKNOWN 0
#define SVO_VOXEL_GRID_LEVEL 1
#define SVO_VOXEL_GRID_OBSTACLE 2
typedef struct svo_voxel_grid_params {
  int up_axis;              /* 0..2 */
  int up_sign;              /* +1 or -1 */
  double origin_a, origin_b; /* finite, map units: the corner of cell (0, 0) */
  int cell_voxels;          /* 1..1024: voxels per cell edge */
  int na, nb;               /* each 1..8192, na*nb <= 2^24 */
  double up_lo, up_hi;      /* the band of heights along UP in map units; not NaN, up_lo <= up_hi, infinities allowed */
  double obstacle_step;     /* >= 0, not NaN: a cell whose span exceeds it is an obstacle */
  int min_count;            /* >= 1 */
} svo_voxel_grid_params;
typedef struct svo_voxel_grid_out { /* na*nb elements each; every pointer but cls may be NULL */
  uint8_t* cls;
  float* top;
  float* bottom;
  uint8_t* intensity;
  uint32_t* n_voxels;
  uint64_t* n_points;
} svo_voxel_grid_out;
/* The defaults above for a map of this voxel size.  Pure; SVO_ERR_INVALID for null params or a voxel_size that is not finite and > 0. */
int svo_voxel_grid_default_params(float voxel_size, svo_voxel_grid_params* params);
/* 32*na*nb; 0 for na or nb < 1.  Pure. */
size_t svo_voxel_grid_workspace_bytes(int na, int nb);
/* Item 4 for a position (a, b) in map units along the grid's axes, so that a caller finds the vehicle's cell by the grid's own rule:
 * k = floor(a / vs) clamped to +-2^21, *ia = floordiv(k - ka0, cell_voxels), likewise *ib (either may be NULL).  Returns 1 when
 * the position is inside the grid, 0 when it is not (ia, ib are written all the same), SVO_ERR_INVALID for null or refused params,
 * a voxel_size that is not finite and > 0, or a NaN position.  Pure. */
int svo_voxel_grid_cell_of(const svo_voxel_grid_params* params, float voxel_size, double a, double b, int* ia, int* ib);
/* DEVICE pointers, asynchronous on svo_stream(ctx): the memsets of the workspace and of the counts, then two launches. */
int svo_voxel_map_grid_dev(svo_voxel_map* map, const svo_voxel_grid_params* params, void* workspace, const svo_voxel_grid_out* out,
                           uint64_t* counts);
/* HOST outputs, synchronous: the workspace and the device outputs are allocated and freed by the call.  out: host pointers (no
 * alignment asked), cls required; counts: 5 u64 on the host or NULL. */
int svo_voxel_map_grid(svo_voxel_map* map, const svo_voxel_grid_params* params, const svo_voxel_grid_out* out, uint64_t* counts);
/* Measurement aid: how the walk issues the two max of item 5.  precheck != 0: a relaxed device-scope load of the word skips the atomic
 * where the word already holds at least the value (words only grow within the launch, so a stale load costs a needless atomic, never
 * a wrong skip).  It cannot change a bit of the outputs or of the workspace.  DESIGN 7j gives the figures and the default. */
int svo_voxel_grid_set_mode(svo_voxel_map* map, int precheck);

/* Ground plan surface: what the grid's class cannot say because it looks at one cell alone (its KNOWN PROPERTIES above).  From the
 * grid's cls and top, per cell: the largest height step to an edge neighbour, the relief (highest minus lowest top) under a
 * vehicle's footprint, how much of the footprint is known ground, and a refined class grid with three new values that every later
 * step can select by its 32-bit mask.  One launch, no workspace; it depends on no thread order and is tested with ==, floats by
 * bit pattern.  cell = ia*nb + ib, as in the grid.  No voxel map is involved.
 *   1. GROUND.  A cell is GROUND iff cls < 32, bit cls of ground_mask is set and top is finite.  A cell whose class bit is set but
 *      whose top is a NaN or infinite is NONFINITE: it gives no height and no support anywhere, and its own cls_out is
 *      SVO_GRID_SURFACE_UNSUPPORTED.
 *   2. Footprint.  rc = footprint_radius / cell_size and r2 = (u64)floor(rc * rc), f64 operations done once on the host; the call is
 *      refused when rc * rc >= 226.  The footprint of a cell is the set of offsets (da, db) with da^2 + db^2 <= r2, at most 15 cells
 *      each way; D(r2) is their number (svo_grid_surface_footprint_cells).  Offsets outside the grid hold nothing.
 *   3. Step.  For a GROUND cell dstep = the maximum of |(double)top - (double)top_n| over its four EDGE neighbours that are inside
 *      the grid and GROUND, one f64 subtraction each; 0 when there is none.  step = (float)dstep; -1.0f for a cell that is not
 *      GROUND.  Diagonal neighbours do not count: the route never cuts a corner.
 *   4. Relief.  For a GROUND cell drelief = (double)hi - (double)lo, hi and lo the largest and smallest top among the GROUND cells of
 *      its footprint (the cell itself is one); where hi == lo it is +0.0, so that -0.0f and +0.0f are one height.  relief =
 *      (float)drelief; -1.0f for a cell that is not GROUND.
 *   5. Support.  support (u16) = the number of GROUND cells in the footprint, written for every cell.
 *   6. Class.  A cell that is neither GROUND nor NONFINITE keeps its class, values >= 32 included.  A GROUND cell takes the first of
 *        (a) dstep > max_step                           -> SVO_GRID_SURFACE_STEP (3)
 *        (b) drelief > max_relief                       -> SVO_GRID_SURFACE_ROUGH (4)
 *        (c) support * 256 < min_support_256 * D (u32)  -> SVO_GRID_SURFACE_UNSUPPORTED (5)
 *      and otherwise keeps its class.  Both comparisons are strict and are made on the f64 values, before the rounding to f32.
 *      +infinity switches (a) or (b) off, min_support_256 = 0 switches (c) off.
 *   7. counts = {n_ground, n_step, n_rough, n_unsupported, n_nonfinite, n_kept}: 6 u64 on the device, or NULL.  n_unsupported leaves
 *      out the NONFINITE cells; n_kept: the GROUND cells that keep their class; n_step + n_rough + n_unsupported + n_kept =
 *      n_ground.  Zeroed on the stream before the launch; one relaxed atomicAdd per workgroup and non-zero counter, counted whether
 *      or not the per-cell outputs are asked for.
 *   8. cls_out is required; step, relief and support may be NULL and are then not written.  cls_out MUST NOT be cls (and no output
 *      may overlap cls or top): neighbouring cells read cls while this one is written.
 *   9. SVO_ERR_INVALID with the argument named, nothing launched and the context usable, for: a null ctx, cls, top, params, out or
 *      cls_out; cls_out == cls; na or nb outside 1..8192 or na*nb > 2^24; ground_mask 0; a cell_size that is not finite and > 0; a
 *      max_step or max_relief that is negative or a NaN; a footprint_radius that is not finite and >= 0, or with rc * rc >= 226;
 *      min_support_256 outside 0..256; a top, step or relief that is not 4-byte aligned, a support not 2-byte, counts not 8-byte
 *      aligned.
 * Both cells of a step are STEP: the entry marks cells, not edges, and the route blocks both.
 * How to use it: put cls_out where cls went, and SVO_GRID_SURFACE_SOURCES into the clearance's source_mask.  The frontiers' free
 * mask stays LEVEL (a STEP cell is no frontier) and the view's opaque mask stays OBSTACLE (a kerb does not block sight).
 * The defaults are NOT tuned on real data: the grid's na and nb, cell_size = cell_voxels * (double)voxel_size, ground_mask =
 * 1 << SVO_VOXEL_GRID_LEVEL, max_step = obstacle_step, footprint_radius = 1.5 * cell_size (r2 = 2), max_relief = 2 * obstacle_step,
 * min_support_256 = 0.
 * The pipeline never calls it by itself; call it between the grid and the clearance. */
#define SVO_GRID_SURFACE_STEP 3
#define SVO_GRID_SURFACE_ROUGH 4
#define SVO_GRID_SURFACE_UNSUPPORTED 5
/* OBSTACLE, STEP, ROUGH and UNSUPPORTED: the clearance's source_mask over cls_out */
#define SVO_GRID_SURFACE_SOURCES ((1u << 2) | (1u << 3) | (1u << 4) | (1u << 5))
typedef struct svo_grid_surface_params {
  int na, nb;               /* each 1..8192, na*nb <= 2^24 */
  uint32_t ground_mask;     /* != 0: bit c set makes class c (0..31) ground */
  double cell_size;         /* finite, > 0: a cell's edge in map units */
  double max_step;          /* >= 0, not NaN; +infinity: no STEP */
  double footprint_radius;  /* finite, >= 0, in map units; (footprint_radius / cell_size)^2 < 226 */
  double max_relief;        /* >= 0, not NaN; +infinity: no ROUGH */
  int min_support_256;      /* 0..256: the share of the footprint that must be ground, in 256ths; 0: no UNSUPPORTED among GROUND cells */
} svo_grid_surface_params;
typedef struct svo_grid_surface_out { /* na*nb elements each; every pointer but cls_out may be NULL */
  uint8_t* cls_out;         /* must not be cls */
  float* step;
  float* relief;
  uint16_t* support;
} svo_grid_surface_out;
/* The defaults above for a grid of svo_voxel_map_grid* over a map of this voxel size.  Pure; SVO_ERR_INVALID for a null pointer, a
 * voxel_size that is not finite and > 0, or a grid whose na, nb, cell_voxels or obstacle_step svo_voxel_map_grid_dev would refuse. */
int svo_grid_surface_default_params(const svo_voxel_grid_params* grid, float voxel_size, svo_grid_surface_params* out);
/* D(r2) of rule 2: 1, 5, 9, 13, 25, 81, 709 for r2 = 0, 1, 2, 4, 8, 25, 225; 0 for r2 > 225, which no accepted call has.  Pure. */
uint32_t svo_grid_surface_footprint_cells(uint32_t r2);
/* DEVICE pointers, asynchronous on svo_stream(ctx).  The counts' memset and the launch are one "grid_surface" profile bracket. */
int svo_grid_surface_dev(svo_ctx* ctx, const uint8_t* cls, const float* top, const svo_grid_surface_params* params,
                         const svo_grid_surface_out* out, uint64_t* counts);
/* HOST cls, top and outputs, synchronous: the device copies are allocated and freed by the call.  out: host pointers (no alignment
 * asked), cls_out required; counts: 6 u64 on the host or NULL. */
int svo_grid_surface(svo_ctx* ctx, const uint8_t* cls, const float* top, const svo_grid_surface_params* params,
                     const svo_grid_surface_out* out, uint64_t* counts);

/* Ground plan clearance: per cell of a u8 class grid the exact squared distance, in cells, to the nearest SOURCE cell, which cell
 * that is, the distance in map units and a robot-radius inflation: what a planner asks a ground plan first.  It works on any
 * na x nb byte grid on the device, cell = ia*nb + ib (the layout of svo_voxel_map_grid*'s cls), is stated in integers, depends
 * on no thread order and is tested with ==.  Two launches: a row pass writes, per cell, the signed offset to the nearest source of
 * its own row into the caller's workspace; a column pass combines the rows.  No voxel map is involved.
 *   1. A cell is a SOURCE iff cls < 32 and bit cls of source_mask is set.  Values >= 32 are never sources.
 *   2. dist2[ia, ib] (u32) is the minimum over all source cells (ja, jb) of (ia-ja)^2 + (ib-jb)^2, provided that minimum is
 *      <= max_dist^2; otherwise it is SVO_GRID_CLEARANCE_NONE = 0xFFFFFFFF.  A source has dist2 = 0.
 *   3. nearest[ia, ib] (u32) is the SMALLEST cell index ja*nb + jb among the sources that attain that minimum, and NONE where dist2
 *      is NONE.  A source names itself.
 *   4. clearance[cell] (f32) = (float)(sqrt((double)dist2) * cell_size): a correctly rounded f64 square root, one f64 product, one
 *      rounding to f32; +infinity where dist2 is NONE.
 *   5. blocked[cell] (u8) is 2 for a source, 1 for a non-source with dist2 <= R2, otherwise 0, where rc = inflate_radius / cell_size
 *      and R2 = (u64)floor(rc * rc) clamped to max_dist^2 (f64, computed once on the host).  inflate_radius 0 blocks sources only.
 *   6. counts = {n_sources, n_reached, n_unreached, n_blocked}: 4 u64 on the device, or NULL.  n_reached: non-sources with
 *      dist2 != NONE; n_unreached: cells with dist2 == NONE; n_blocked: cells of value 1 (counted whether or not blocked is asked
 *      for).  The three first sum to na*nb.  Zeroed on the stream before the first launch; one relaxed atomicAdd per workgroup and
 *      non-zero counter.
 *   7. dist2 is required, every other output may be NULL and is then not written.  workspace: svo_grid_clearance_workspace_bytes(na,
 *      nb) = 4*na*nb bytes of device memory, 4-byte aligned; its contents before the call are meaningless, afterwards it holds the
 *      row pass's int32 offsets.  cls is only read; it must not overlap the workspace or an output.
 *   8. SVO_ERR_INVALID with the argument named, and nothing launched, for: a null ctx, cls, params, workspace, out or out->dist2;
 *      na or nb outside 1..8192 or na*nb > 2^24; source_mask 0; max_dist outside 1..8191; a cell_size that is not finite and > 0; an
 *      inflate_radius that is not finite and >= 0; a workspace, dist2, nearest or clearance that is not 4-byte aligned, counts not
 *      8-byte aligned.  The context stays usable.
 * max_dist is part of the contract in the way SVO_VOXEL_MAX_PROBES is: it bounds what a cell far from every source costs (2 *
 * max_dist + 1 cells of its row and as many rows), and cells farther than that from every source are NONE, not "far".
 * EXACTNESS.  A source at distance <= max_dist lies inside the +-max_dist square the two passes cover, everything outside is
 * farther.  The sources that attain a cell's minimum and have the smallest row ja are, in that row, the nearest to column ib, so the
 * row pass's choice (the nearer of ib-g and ib+g, the left one at equal g) is among them and is the one with the smallest index.
 * The defaults are NOT tuned on real data: the grid's na and nb, cell_size = cell_voxels * (double)voxel_size, source_mask =
 * 1 << SVO_VOXEL_GRID_OBSTACLE, max_dist 64 cells, inflate_radius 0.
 * The pipeline never computes a clearance by itself; call it after the grid it reads. */
#define SVO_GRID_CLEARANCE_NONE 0xFFFFFFFFu
typedef struct svo_grid_clearance_params {
  int na, nb;             /* each 1..8192, na*nb <= 2^24 */
  uint32_t source_mask;   /* != 0: bit c set makes class c (0..31) a source */
  int max_dist;           /* 1..8191, in cells */
  double cell_size;       /* finite, > 0: a cell's edge in map units */
  double inflate_radius;  /* finite, >= 0, in map units */
} svo_grid_clearance_params;
typedef struct svo_grid_clearance_out { /* na*nb elements each; every pointer but dist2 may be NULL */
  uint32_t* dist2;
  uint32_t* nearest;
  float* clearance;
  uint8_t* blocked;
} svo_grid_clearance_out;
/* The defaults above for a grid of svo_voxel_map_grid* over a map of this voxel size.  Pure; SVO_ERR_INVALID for a null pointer, a
 * voxel_size that is not finite and > 0, or a grid whose na, nb or cell_voxels svo_voxel_map_grid_dev would refuse. */
int svo_grid_clearance_default_params(const svo_voxel_grid_params* grid, float voxel_size, svo_grid_clearance_params* out);
/* 4*na*nb; 0 for na or nb < 1.  Pure. */
size_t svo_grid_clearance_workspace_bytes(int na, int nb);
/* DEVICE pointers, asynchronous on svo_stream(ctx): the counts' memset, then two launches. */
int svo_grid_clearance_dev(svo_ctx* ctx, const uint8_t* cls, const svo_grid_clearance_params* params, void* workspace,
                           const svo_grid_clearance_out* out, uint64_t* counts);
/* HOST cls and outputs, synchronous: the device copies and the workspace are allocated and freed by the call.  out: host pointers
 * (no alignment asked), dist2 required; counts: 4 u64 on the host or NULL. */
int svo_grid_clearance(svo_ctx* ctx, const uint8_t* cls, const svo_grid_clearance_params* params, const svo_grid_clearance_out* out,
                       uint64_t* counts);

/* Ground plan route: from every cell of a byte grid the cost of the cheapest way to a goal cell that stays off the impassable cells
 * and pays for coming near an obstacle, the first move of that way, and the cells of the way from given start cells: what a planner
 * asks a ground plan second.  Integers only; a converged result is the unique fixed point of the relaxation (positive integer
 * weights), depends on no thread order and is tested with ==.  cell = ia*nb + ib, as in the grid and the clearance.
 * INPUTS (device memory for the _dev entry): blocked, na*nb u8, required: a cell is passable iff its byte is 0 (the clearance's
 * blocked fits as it is); dist2, na*nb u32 or NULL (the clearance's dist2, 0xFFFFFFFF included); goals, n_goals (1..65536) u32 cell
 * indices; starts, n_starts (0..4096) u32 cell indices, NULL with n_starts == 0.
 *   1. pen[v] = near_weight * (near_r2 - dist2[v]) where dist2 is given and dist2[v] < near_r2, else 0 (NONE is far, a NULL dist2 is
 *      far everywhere).
 *   2. The eight neighbours are coded k = 0..7 in raster order of (dia, dib): (-1,-1) (-1,0) (-1,+1) (0,-1) (0,+1) (+1,-1) (+1,0)
 *      (+1,+1).  A move from v to u is allowed iff both cells are inside the grid and passable and, for a diagonal, both cells it
 *      passes between, (ia+dia, ib) and (ia, ib+dib), are passable (no corner cutting).  It costs w * (16 + pen[u]), w = 5 along an
 *      axis and 7 on a diagonal: the 5-7 chamfer with the penalty of the cell entered.  One step costs less than 2^23.
 *   3. A goal index >= na*nb or on an impassable cell is ignored; the others have cost 0.
 *   4. cost[v] (u32, required) is the cheapest sum of move costs from v to any used goal if that sum is <= max_cost, else
 *      SVO_GRID_ROUTE_NONE = 0xFFFFFFFF; impassable cells are NONE.  Every prefix of a route within the cap is within the cap, so the
 *      capped field is the true one truncated; candidates never exceed 0x7F000000 + 2^23, so u32 arithmetic does not wrap.
 *   5. next[v] (u8, optional) is 8 at a used goal, otherwise the smallest k whose move is allowed and has cost[u_k] + step ==
 *      cost[v], and 255 where cost is NONE.  Following next strictly lowers cost, so it ends at a goal.
 *   6. Paths (optional, all three or none): path n_starts x max_path u32, path_len n_starts u32, path_status n_starts u8.  Row i holds
 *      the cells from starts[i] along next to the goal, both ends included; path_len[i] is the full number of cells, only the first
 *      max_path are written and row entries past the written ones are not touched.  Status SVO_GRID_ROUTE_OK, _TRUNCATED (len >
 *      max_path), _UNREACHED (cost NONE; len 0), _OUT_OF_GRID (len 0) or _NOT_CONVERGED (len 0).
 *   7. counts: 8 u64 on the device, or NULL: {n_goals_used, n_reached, n_unreached, n_impassable, converged, rounds_run, 0, 0}.  They
 *      are zeroed on the stream and every add is a relaxed one behind everything queued before the call.  n_reached counts passable
 *      cells with a cost, goals included; n_reached + n_unreached + n_impassable = na*nb; n_goals_used counts list entries, so a
 *      duplicate counts twice.
 *   8. The call enqueues max_rounds relaxation rounds.  converged is 1 iff the last round that ran changed nothing.  If it is 0,
 *      cost holds upper bounds whose bits may depend on timing, next and path are not written, every path_len is 0 and every status
 *      _NOT_CONVERGED, and the three cell counts stay 0.  rounds_run (the last round of this call in which a tile had work) is
 *      reported but may depend on how workgroups interleave.  A call with resume = 1, the same blocked, dist2, goals and params and
 *      the same workspace and cost buffers untouched since, continues where the earlier call stopped; repeating such calls reaches
 *      converged = 1 and the unique field.
 *   9. workspace: svo_grid_route_workspace_bytes(na, nb) bytes of device memory, 8-byte aligned, contents meaningless on entry
 *      unless resume.  blocked, dist2, goals and starts are only read and must not overlap an output.
 *  10. SVO_ERR_INVALID with the argument named, nothing launched and the context still usable, for: a null ctx, blocked, params,
 *      goals, workspace, out or cost; every range of the fields below (max_path only when n_starts > 0); n_goals outside 1..65536,
 *      n_starts outside 0..4096; starts NULL with n_starts > 0; any of path, path_len, path_status NULL while another is not, or
 *      non-NULL with n_starts == 0; cost, dist2, goals, starts, path or path_len off 4 bytes; workspace or counts off 8 bytes.
 * UNIQUENESS.  With positive integer step costs the equations cost[goal] = 0, cost[v] = min over allowed moves of cost[u] + step have
 * one solution, the shortest-route cost; relaxation only lowers a word towards it and never below, in whatever order cells are
 * relaxed.  That is what lets the tiled parallel form be compared with == against Dijkstra.
 * The defaults are NOT tuned on real data: the clearance's na and nb, near_r2 0, near_weight 0, max_cost 0x7F000000, max_rounds 64,
 * max_path 4096, resume 0.  64 rounds cover ground plans; a maze takes resume.
 * The pipeline never computes a route by itself; call it after the clearance it reads. */
#define SVO_GRID_ROUTE_NONE 0xFFFFFFFFu
#define SVO_GRID_ROUTE_MAX_COST 0x7F000000u
enum { SVO_GRID_ROUTE_OK = 0, SVO_GRID_ROUTE_TRUNCATED = 1, SVO_GRID_ROUTE_UNREACHED = 2, SVO_GRID_ROUTE_OUT_OF_GRID = 3,
       SVO_GRID_ROUTE_NOT_CONVERGED = 4 };
typedef struct svo_grid_route_params {
  int na, nb;           /* each 1..8192, na*nb <= 2^24 */
  uint32_t near_r2;     /* 0..2^26: squared radius, in cells, inside which the penalty applies */
  uint32_t near_weight; /* near_weight * near_r2 <= 2^20: penalty per unit of near_r2 - dist2 */
  uint32_t max_cost;    /* 1..0x7F000000: cap on a cell's cost */
  int max_rounds;       /* 1..4096: relaxation rounds this call enqueues */
  int max_path;         /* 1..2^20, read only when n_starts > 0: cells written per path */
  int resume;           /* 0 or 1: continue an earlier call's field */
} svo_grid_route_params;
typedef struct svo_grid_route_out { /* every pointer but cost may be NULL; path, path_len and path_status only together */
  uint32_t* cost;       /* na*nb */
  uint8_t* next;        /* na*nb */
  uint32_t* path;       /* n_starts * max_path */
  uint32_t* path_len;   /* n_starts */
  uint8_t* path_status; /* n_starts */
} svo_grid_route_out;
/* The defaults above for the grid of a clearance.  Pure; SVO_ERR_INVALID for a null pointer or an na, nb the clearance refuses. */
int svo_grid_route_default_params(const svo_grid_clearance_params* clearance, svo_grid_route_params* out);
/* Bytes of the workspace: a header, two activity words per tile and one byte per cell; 0 for na or nb < 1.  Pure. */
size_t svo_grid_route_workspace_bytes(int na, int nb);
/* DEVICE pointers, asynchronous on svo_stream(ctx).  Everything it enqueues is one "grid_route" profile bracket. */
int svo_grid_route_dev(svo_ctx* ctx, const uint8_t* blocked, const uint32_t* dist2, const svo_grid_route_params* params,
                       const uint32_t* goals, int n_goals, const uint32_t* starts, int n_starts, void* workspace,
                       const svo_grid_route_out* out, uint64_t* counts);
/* HOST arrays and outputs (no alignment asked), synchronous: one device allocation for the call, freed after the stream is drained.
 * counts: 8 u64 on the host or NULL.  resume = 1 is refused: the workspace does not outlive the call. */
int svo_grid_route(svo_ctx* ctx, const uint8_t* blocked, const uint32_t* dist2, const svo_grid_route_params* params,
                   const uint32_t* goals, int n_goals, const uint32_t* starts, int n_starts, const svo_grid_route_out* out,
                   uint64_t* counts);

/* Ground plan frontiers: the passable cells of known ground that touch ground nobody has seen yet, grouped into connected pieces,
 * each with its size, bounds, a representative cell and its cheapest cell: where a vehicle that builds its own map goes next, and
 * what the route takes as its goals.  Integers only, no dependence on thread order, tested with ==.  cell = ia*nb + ib, as in the
 * grid, the clearance and the route.
 * INPUTS (device memory for the _dev entry): cls, na*nb u8, required (svo_voxel_map_grid*'s cls or any other class grid); blocked,
 * na*nb u8 or NULL (the clearance's blocked); cost, na*nb u32 or NULL (a route's cost field, for instance one whose only goal is the
 * vehicle's cell).
 *   1. A cell is FREE iff cls < 32, bit cls of free_mask is set, and blocked is NULL or blocked[cell] == 0.  A cell is UNKNOWN iff
 *      cls < 32 and bit cls of unknown_mask is set.  Values >= 32 are neither.
 *   2. A cell is a FRONTIER CELL iff it is FREE and at least one of its four edge neighbours inside the grid is UNKNOWN.  The outside
 *      of the grid is not unknown; a diagonal neighbour does not count.
 *   3. A frontier is an 8-connected component of frontier cells.
 *   4. Per frontier: size, the number of cells; first_cell, the smallest cell index; sum_a, sum_b, the sums of ia and of ib (at most
 *      2^37); min_a, max_a, min_b, max_b, the bounds.
 *   5. rep_cell: with (ca, cb) = (sum_a / size, sum_b / size), integer division, the member cell with the smallest (ia-ca)^2 +
 *      (ib-cb)^2, ties to the smallest index.  It is always a member, so it is FREE; the centroid itself need not be one.
 *   6. best_cell, best_cost: the member cell with the smallest cost among the members whose cost != 0xFFFFFFFF, ties to the smallest
 *      index, and its cost.  Both are 0xFFFFFFFF when cost is NULL or no member has a cost.
 *   7. A frontier is KEPT iff size >= min_size.  Kept frontiers are ranked by ascending first_cell.  Record i describes rank i for i <
 *      min(n_kept, max_frontiers); records past that are not touched.
 *   8. goal_cells[i] is rep_cell of rank i for i < min(n_kept, max_frontiers); all other entries up to max_frontiers are written as
 *      0xFFFFFFFF, which svo_grid_route_dev ignores by its rule 3: the array goes into the route as it is, with n_goals =
 *      max_frontiers and no count read back.
 *   9. label[cell] is the rank of its frontier for a cell of a kept frontier, also where the rank is >= max_frontiers, and
 *      0xFFFFFFFF for every other cell.
 *  10. counts: 8 u64 on the device, or NULL: {n_free, n_unknown, n_frontier_cells, n_frontiers, n_kept, n_written, n_kept_cells, 0}.
 *      Zeroed on the stream; relaxed adds only.  n_written = min(n_kept, max_frontiers).
 *  11. workspace: svo_grid_frontier_workspace_bytes(na, nb, max_frontiers) bytes of device memory, 8-byte aligned, contents
 *      meaningless on entry.  The function is pure, computes in size_t and returns 0 for a refused shape; the size is
 *        256 + 64 * max_frontiers + round8(4 * ceil(na*nb / 256)) + round8(12 * na*nb),   round8(x) = x rounded up to 8,
 *      which is at most 16 * na*nb + 64 * max_frontiers + 4096.
 *  12. SVO_ERR_INVALID with the argument named, nothing launched and the context still usable, looked for in this order: a null
 *      ctx; a null cls, params, workspace, out; na, nb outside 1..8192, na*nb > 2^24; free_mask 0; unknown_mask 0; min_size
 *      outside 1..2^24; max_frontiers outside 1..65536; masks that share a bit; frontiers, goal_cells and label all NULL; cost,
 *      label, goal_cells off 4 bytes; frontiers, workspace, counts off 8 bytes.  cls, blocked and cost are only read; they must not
 *      overlap an output or the workspace.
 * The defaults are NOT tuned on real data: the clearance's na and nb, free_mask = 1 << SVO_VOXEL_GRID_LEVEL, unknown_mask =
 * 1 << SVO_VOXEL_GRID_UNKNOWN, min_size 3, max_frontiers 1024.
 * The pipeline never calls the entry by itself; call it after the clearance (and, for best_cell, the route) it reads, before the
 * route that takes goal_cells. */
#define SVO_GRID_FRONTIER_NONE 0xFFFFFFFFu
typedef struct svo_grid_frontier_params {
  int na, nb;             /* each 1..8192, na*nb <= 2^24 */
  uint32_t free_mask;     /* != 0: bit c set makes class c (0..31) FREE */
  uint32_t unknown_mask;  /* != 0, no bit in common with free_mask */
  uint32_t min_size;      /* 1..2^24: smallest frontier kept, in cells */
  int max_frontiers;      /* 1..65536: records written; the route's n_goals limit */
} svo_grid_frontier_params;
typedef struct svo_grid_frontier {        /* 48 bytes, 8-byte aligned */
  uint32_t first_cell, size, rep_cell, best_cell, best_cost;
  uint16_t min_a, max_a, min_b, max_b;
  uint32_t reserved;                      /* 0 */
  uint64_t sum_a, sum_b;
} svo_grid_frontier;
typedef struct svo_grid_frontier_out {    /* each may be NULL, but not all three */
  svo_grid_frontier* frontiers;           /* max_frontiers records */
  uint32_t* goal_cells;                   /* max_frontiers */
  uint32_t* label;                        /* na*nb */
} svo_grid_frontier_out;
/* The defaults above for the grid of a clearance.  Pure; SVO_ERR_INVALID for a null pointer or an na, nb the clearance refuses. */
int svo_grid_frontier_default_params(const svo_grid_clearance_params* clearance, svo_grid_frontier_params* out);
/* Item 11's size; 0 for a shape or a max_frontiers that item 12 refuses.  Pure. */
size_t svo_grid_frontier_workspace_bytes(int na, int nb, int max_frontiers);
/* DEVICE pointers, asynchronous on svo_stream(ctx).  Everything it enqueues is one "grid_frontier" profile bracket. */
int svo_grid_frontiers_dev(svo_ctx* ctx, const uint8_t* cls, const uint8_t* blocked, const uint32_t* cost,
                           const svo_grid_frontier_params* params, void* workspace, const svo_grid_frontier_out* out, uint64_t* counts);
/* HOST arrays and outputs (no alignment asked), synchronous: one device allocation for the call, freed after the stream is drained
 * whatever failed.  The caller's frontiers are copied up first, so that the records item 7 leaves untouched come back as they were.
 * counts: 8 u64 on the host or NULL. */
int svo_grid_frontiers(svo_ctx* ctx, const uint8_t* cls, const uint8_t* blocked, const uint32_t* cost,
                       const svo_grid_frontier_params* params, const svo_grid_frontier_out* out, uint64_t* counts);
/* Measurement aid: combine != 0 (the state of a new context) lets runs of equal rank along a wavefront add into a frontier's
 * statistics once; 0 makes every cell issue its own atomics.  It cannot change a bit of an output.  DESIGN 7m gives the figures. */
int svo_grid_frontier_set_mode(svo_ctx* ctx, int combine);

/* Ground plan view: standing on each of a list of candidate cells, how much ground would be seen, how much of it is ground nobody
 * has seen yet, and what that is worth against the cost of getting there; the candidates ranked and the best one named: which of the
 * frontiers' goal_cells a vehicle that explores should drive to.  Integers only, no dependence on thread order, tested with ==.
 * cell = ia*nb + ib, as in the grid, the clearance, the route and the frontiers.
 * INPUTS (device memory for the _dev entry): cls, na*nb u8, required (svo_voxel_map_grid*'s cls or any other class grid); views,
 * n_views (1..4096) u32 cell indices (the frontiers' goal_cells fit as they are, padding included); cost, na*nb u32 or NULL (a
 * route's cost field, for instance the one whose only goal is the vehicle's cell).
 *   1. A cell is OPAQUE iff cls < 32 and bit cls of opaque_mask is set.  It is GAIN iff cls < 32 and bit cls of gain_mask is set.
 *      Values >= 32 are neither.  The masks may share a bit: with the UNKNOWN bit in both, a line ends at the first unknown cell and
 *      only the first layer of unknown ground counts (the conservative gain); with it in gain_mask only, unknown ground is looked
 *      through (the optimistic gain).
 *   2. View i is USED iff views[i] < na*nb and that cell is not OPAQUE.  Every other entry is IGNORED: 0xFFFFFFFF padding, an index
 *      outside the grid, a view standing in a wall.  Duplicates are each used.
 *   3. The line from V = (va, vb) to T = (ta, tb): da = ta - va, db = tb - vb, n = max(|da|, |db|), and for i = 0..n
 *        L_i = (va + sgn(da) * floor((2*i*|da| + n) / (2n)), vb + sgn(db) * floor((2*i*|db| + n) / (2n))).
 *      L_0 = V, L_n = T; the major coordinate moves one cell per step; a tie of the minor coordinate rounds away from V.  The rule
 *      commutes with the grid's eight symmetries; it is not symmetric in V and T.  Every L_i lies in the bounding box of V and T.
 *   4. T is VISIBLE from V iff T is inside the grid, da^2 + db^2 <= max_range^2, no L_i with 1 <= i <= n-1 is OPAQUE, and for every
 *      step L_(i-1) -> L_i, 1 <= i <= n, that changes both coordinates, not both cells it passes between, (a_i, b_(i-1)) and
 *      (a_(i-1), b_i), are OPAQUE (no sight through a closed corner: the route's no-corner-cutting rule for light).  T itself may be
 *      OPAQUE: one sees the face of a wall.  V is visible from itself.  Visibility is defined per target by its own line; "visible
 *      iff the predecessor is visible" is a different function.
 *   5. Record i (svo_grid_view_rec), for a used view: cell; n_visible; n_gain, the visible GAIN cells; n_opaque, the visible OPAQUE
 *      cells; cost = cost[cell], or 0xFFFFFFFF when cost is NULL; score; reserved = 0.  For an ignored view: cell = 0xFFFFFFFF, the
 *      three tallies 0, cost = 0xFFFFFFFF, score = 0.  All n_views records are written.
 *   6. score of a used view: 0 when cost is given and cost[cell] == 0xFFFFFFFF (unreachable).  Otherwise with g = gain_weight *
 *      n_gain in u64 (below 2^34) and c = cost[cell] / cost_div, or 0 when cost is NULL: score = g > c ? min(g - c, 0xFFFFFFFE) : 0.
 *   7. order[r] (u32, n_views entries) is the view index of rank r: descending score, ties to the smaller index.  Ignored views are
 *      ranked too, with score 0.
 *   8. best (4 u32) is {cell, index, score, n_gain} of order[0] when its score is > 0, else {0xFFFFFFFF, 0xFFFFFFFF, 0, 0}.  Its
 *      first word goes into svo_grid_route_dev as goals with n_goals = 1; the route ignores 0xFFFFFFFF by its rule 3.
 *   9. seen[cell] (u32, na*nb, optional) is the smallest index of a used view from which the cell is visible, 0xFFFFFFFF for a cell
 *      that no used view sees.
 *  10. counts: 8 u64 on the device, or NULL: {n_used, n_ignored, n_in_range, n_visible, n_gain, n_covered, n_gain_covered, 0}.
 *      Zeroed on the stream; relaxed adds only.  n_in_range counts the targets inside the grid and the range summed over the used
 *      views, V included; n_visible and n_gain are the records' sums; n_covered counts the cells seen by at least one used view and
 *      n_gain_covered the GAIN cells among them, whether or not seen is asked for (the workspace holds the array then).
 *  11. workspace: svo_grid_view_workspace_bytes(na, nb, n_views) bytes of device memory, 8-byte aligned, contents meaningless on
 *      entry: a header, 16 bytes per view and one u32 per cell.  The function is pure, computes in size_t and returns 0 for a
 *      refused shape; the size is
 *        256 + 16 * n_views + round8(4 * na*nb),   round8(x) = x rounded up to 8.
 *  12. SVO_ERR_INVALID with the argument named, nothing launched and the context still usable, looked for in this order: a null
 *      ctx; a null cls, params, views, workspace, out; na, nb outside 1..8192, na*nb > 2^24; opaque_mask 0; gain_mask 0; max_range
 *      outside 1..255; gain_weight outside 1..65536; cost_div outside 1..2^31; n_views outside 1..4096; records, order, best and
 *      seen all NULL; views, cost, order, best, seen off 4 bytes; records, workspace, counts off 8 bytes.  cls, views and cost are
 *      only read; they must not overlap an output or the workspace.
 * The defaults are NOT tuned on real data: the clearance's na and nb, opaque_mask = 1 << SVO_VOXEL_GRID_OBSTACLE, gain_mask =
 * 1 << SVO_VOXEL_GRID_UNKNOWN, max_range = min(the clearance's max_dist, 255), gain_weight 16, cost_div 1.
 * The pipeline never calls the entry by itself; call it after the frontiers whose goal_cells it reads and the route whose cost it
 * reads, before the route that takes best. */
#define SVO_GRID_VIEW_NONE 0xFFFFFFFFu
#define SVO_GRID_VIEW_MAX_VIEWS 4096
typedef struct svo_grid_view_params {
  int na, nb;             /* each 1..8192, na*nb <= 2^24 */
  uint32_t opaque_mask;   /* != 0: bit c set makes class c (0..31) OPAQUE */
  uint32_t gain_mask;     /* != 0: bit c set makes class c (0..31) GAIN; may share bits with opaque_mask */
  int max_range;          /* 1..255, in cells */
  uint32_t gain_weight;   /* 1..65536: score per visible GAIN cell */
  uint32_t cost_div;      /* 1..2^31: the cost is divided by it before it is taken off */
} svo_grid_view_params;
typedef struct svo_grid_view_rec {        /* 32 bytes, 8-byte aligned */
  uint32_t cell, n_visible, n_gain, n_opaque, cost, score;
  uint32_t reserved[2];                   /* 0 */
} svo_grid_view_rec;
typedef struct svo_grid_view_out {        /* each may be NULL, but not all four */
  svo_grid_view_rec* records;             /* n_views records */
  uint32_t* order;                        /* n_views */
  uint32_t* best;                         /* 4 */
  uint32_t* seen;                         /* na*nb */
} svo_grid_view_out;
/* The defaults above for the grid of a clearance.  Pure; SVO_ERR_INVALID for a null pointer or an na, nb the clearance refuses. */
int svo_grid_view_default_params(const svo_grid_clearance_params* clearance, svo_grid_view_params* out);
/* Item 11's size; 0 for a shape or an n_views that item 12 refuses.  Pure. */
size_t svo_grid_view_workspace_bytes(int na, int nb, int n_views);
/* DEVICE pointers, asynchronous on svo_stream(ctx).  Everything it enqueues is one "grid_view" profile bracket. */
int svo_grid_view_dev(svo_ctx* ctx, const uint8_t* cls, const uint32_t* views, int n_views, const uint32_t* cost,
                      const svo_grid_view_params* params, void* workspace, const svo_grid_view_out* out, uint64_t* counts);
/* HOST arrays and outputs (no alignment asked), synchronous: one device allocation for the call, freed after the stream is drained
 * whatever failed.  counts: 8 u64 on the host or NULL. */
int svo_grid_view(svo_ctx* ctx, const uint8_t* cls, const uint32_t* views, int n_views, const uint32_t* cost,
                  const svo_grid_view_params* params, const svo_grid_view_out* out, uint64_t* counts);
/* Measurement aid: staged != 0 (the state of a new context) lets a view's workgroup walk its lines over two bit planes of the
 * window staged in LDS; 0 makes every step of a line read cls from global memory.  It cannot change a bit of an output.  DESIGN 7n
 * gives the figures. */
int svo_grid_view_set_mode(svo_ctx* ctx, int staged);

/* Ground plan waypoints: from a route's paths, one entry per cell of a 5-7 chamfer staircase, the few cells between which a vehicle
 * may drive in straight lines: what a planner hands to a controller.  Integers apart from one optional length, no dependence on thread
 * order, tested with ==.  cell = ia*nb + ib, as in the grid, the clearance, the route, the frontiers and the view.
 * INPUTS (device memory for the _dev entry): blocked, na*nb u8, required: passable iff 0 (the clearance's blocked as it is); dist2,
 * na*nb u32 or NULL (the clearance's dist2); path, n_paths x path_stride u32 (the route's path; path_stride is the route's max_path);
 * path_len, n_paths u32; path_status, n_paths u8 or NULL (NULL: every path counts as OK); n_paths 1..4096.
 *   1. A cell is SOLID iff blocked[v] != 0, or dist2 is given and dist2[v] < min_dist2.  0xFFFFFFFF is far; min_dist2 = 0 switches
 *      the second clause off.
 *   2. m = min(path_len[p], path_stride) cells of path p are available.  Path p is USED iff path_status is NULL or its status is
 *      SVO_GRID_ROUTE_OK or _TRUNCATED, and m >= 1, and every one of its first m entries is < na*nb.  Otherwise it is SKIPPED:
 *      way_len = 0, length = 0.0, its rows of way and way_index are not touched, and its status is SVO_GRID_WAY_BAD_CELL where the
 *      reason is an entry outside the grid (a status the route would refuse comes first, then m = 0, then the entries) and
 *      SVO_GRID_WAY_SKIPPED otherwise.  Adjacency of consecutive entries is not checked: any list of in-grid cells is accepted.
 *   3. The line from V = (va, vb) to T = (ta, tb): da = ta - va, db = tb - vb, n = max(|da|, |db|), and for i = 0..n
 *        L_i = (va + sgn(da) * floor((2*i*|da| + n) / (2n)), vb + sgn(db) * floor((2*i*|db| + n) / (2n))).
 *      L_0 = V, L_n = T; the major coordinate moves one cell per step; a tie of the minor coordinate rounds away from V.  The rule
 *      commutes with the grid's eight symmetries; it is not symmetric in V and T.  Every L_i lies in the bounding box of V and T.
 *      (The view's rule 3, word for word.)  V is the waypoint already chosen, T the candidate.
 *   4. CLEAR(V, T) holds iff n <= max_look, neither V nor T is SOLID, no L_i with 1 <= i <= n-1 is SOLID, and for every step L_(i-1)
 *      -> L_i, 1 <= i <= n, that changes both coordinates, NEITHER of the two cells it passes between, (a_i, b_(i-1)) and (a_(i-1),
 *      b_i), is SOLID.  The last clause is the route's rule 2; the view's rule 4 stops only at a corner closed on both sides.  For
 *      n = 1 CLEAR is exactly the route's allowed move; for n = 0 it holds iff V is not SOLID.
 *   5. The waypoints are path indices k_0 < k_1 < ... < k_(w-1) with k_0 = 0.  While k_t < m-1: k_(t+1) is the LARGEST j with
 *      k_t + 1 < j <= min(k_t + max_look, m-1) and CLEAR(path[k_t], path[j]); if there is none, k_(t+1) = k_t + 1, and that step is
 *      FORCED iff CLEAR(path[k_t], path[k_t + 1]) is false.  k_(w-1) = m-1, and m = 1 gives w = 1.  CLEAR is decided per candidate by
 *      its own line: "the largest clear j" is a different function from "the last j before the first failure".  For a path the route
 *      made from the same blocked, with min_dist2 = 0, no step is FORCED (rule 4 at n = 1).
 *   6. OUTPUTS (svo_grid_waypoint_out).  way, n_paths x max_way u32: way[p][t] = path[p][k_t] for t < max_way; later entries are not
 *      touched.  way_index, the same shape: k_t.  way_len, n_paths u32: w, the full number.  way_status, n_paths u8: for a used path
 *      a sum of SVO_GRID_WAY_PATH_TRUNCATED = 1 (path_len > path_stride, so the last waypoint is not the goal) and SVO_GRID_WAY_FULL
 *      = 2 (w > max_way), so 0 is OK; SVO_GRID_WAY_SKIPPED = 4 and SVO_GRID_WAY_BAD_CELL = 5 for a skipped one.  length, n_paths f64:
 *      s = 0.0; for t = 1..w-1 in order s = s + sqrt((double)(da^2 + db^2)) between k_(t-1) and k_t, a correctly rounded f64 square
 *      root as in the clearance's rule 4; length = s * cell_size, one product.  All w segments count, those past max_way too.
 *   7. counts: 8 u64 on the device, or NULL: {n_used, n_skipped, n_cells_in, n_waypoints, n_forced, n_full, max_d2, 0}.  Zeroed on
 *      the stream; relaxed adds, a relaxed max for max_d2.  n_skipped includes the paths refused for a bad cell; n_cells_in is the sum
 *      of m over used paths; n_waypoints the sum of w; n_forced the number of FORCED steps; n_full the number of paths with _FULL;
 *      max_d2 the largest da^2 + db^2 of any segment.
 *   8. SVO_ERR_INVALID with the argument named, nothing launched and the context still usable, looked for in this order: a null
 *      ctx; a null blocked, params, path, path_len, out; na, nb outside 1..8192, na*nb > 2^24; path_stride outside 1..2^20; max_look
 *      outside 1..255; min_dist2 > 2^26; max_way outside 1..2^20; a cell_size that is not finite and > 0; n_paths outside 1..4096;
 *      one of way and way_len NULL and the other not, every output NULL; dist2, path, path_len, way, way_index, way_len off 4 bytes;
 *      length, counts off 8 bytes.  The inputs are only read; they must not overlap an output.
 *   9. No workspace: a path's workgroup keeps what it needs in registers and LDS.
 * The defaults are NOT tuned on real data: the route's na and nb, path_stride = the route's max_path, max_look 64, min_dist2 0, max_way
 * 256, the clearance's cell_size.
 * The pipeline never calls the entry by itself; call it after the route whose paths it reads. */
#define SVO_GRID_WAY_MAX_PATHS 4096
enum { SVO_GRID_WAY_OK = 0, SVO_GRID_WAY_PATH_TRUNCATED = 1, SVO_GRID_WAY_FULL = 2, SVO_GRID_WAY_SKIPPED = 4, SVO_GRID_WAY_BAD_CELL = 5 };
typedef struct svo_grid_waypoint_params {
  int na, nb;          /* each 1..8192, na*nb <= 2^24 */
  int path_stride;     /* 1..2^20: entries between two rows of path; the route's max_path */
  int max_look;        /* 1..255: the longest segment in cells (Chebyshev) and in path entries */
  uint32_t min_dist2;  /* 0..2^26: with dist2, cells nearer than this to an obstacle are SOLID */
  int max_way;         /* 1..2^20: waypoints written per path */
  double cell_size;    /* finite, > 0: a cell's edge in map units, for length */
} svo_grid_waypoint_params;
typedef struct svo_grid_waypoint_out { /* each may be NULL, but not all; way and way_len only together */
  uint32_t* way;        /* n_paths * max_way */
  uint32_t* way_index;  /* n_paths * max_way */
  uint32_t* way_len;    /* n_paths */
  uint8_t* way_status;  /* n_paths */
  double* length;       /* n_paths */
} svo_grid_waypoint_out;
/* The defaults above for a route and the clearance it read.  Pure; SVO_ERR_INVALID for a null pointer, an na, nb or max_path the
 * route refuses or a cell_size the clearance refuses. */
int svo_grid_waypoints_default_params(const svo_grid_route_params* route, const svo_grid_clearance_params* clearance,
                                      svo_grid_waypoint_params* out);
/* DEVICE pointers, asynchronous on svo_stream(ctx): the counts' memset and one launch, one "grid_waypoints" profile bracket. */
int svo_grid_waypoints_dev(svo_ctx* ctx, const uint8_t* blocked, const uint32_t* dist2, const uint32_t* path, const uint32_t* path_len,
                           const uint8_t* path_status, int n_paths, const svo_grid_waypoint_params* params,
                           const svo_grid_waypoint_out* out, uint64_t* counts);
/* HOST arrays and outputs (no alignment asked), synchronous: one device allocation for the call, freed after the stream is drained
 * whatever failed.  The caller's way and way_index are copied up first, so that what rules 2 and 6 leave untouched comes back as it
 * was.  counts: 8 u64 on the host or NULL. */
int svo_grid_waypoints(svo_ctx* ctx, const uint8_t* blocked, const uint32_t* dist2, const uint32_t* path, const uint32_t* path_len,
                       const uint8_t* path_status, int n_paths, const svo_grid_waypoint_params* params,
                       const svo_grid_waypoint_out* out, uint64_t* counts);

/* ------------------------------------------------------------------- a8 --
 * ImageProcessor::triangulate_stereo's reprojection loop
 * (src/image_processor.cpp:178-207): keep i iff disp[i] > 0; X = pose * Q * [x y d 1]^T,
 * de-homogenised.  pose16: row-major 4x4 float camera->world.  Output order =
 * input order (stable).  kept_xy: n x 2, xyz: n x 3, kept_index: n (index into the
 * input list) or NULL. */
int svo_triangulate(svo_ctx* ctx, const float* xy, const float* disp, int n, const float* pose16,
                    float focal, float cx, float cy, float baseline,
                    float* kept_xy, float* xyz, int* kept_index, int* n_kept);

/* ------------------------------------------------------------------- a3 --
 * cv::calcOpticalFlowPyrLK(prev, next, pts, out, status, err, Size(21,21), 3,
 * TermCriteria(COUNT+EPS,30,0.01), 0, 1e-2)
 * (src/feature_tracker.cpp:23-26).  out: n x 2, status: n bytes. */
int svo_lk_track(svo_ctx* ctx, const uint8_t* prev, const uint8_t* next, int width, int height,
                 int row_stride, const float* xy, int n, float* out_xy, uint8_t* status);
/* The 4-level pyramid the tracker uses (pyrDown chain), for parity taps.
 * levels: concatenated level images, level l has size ((w+2^l-1)>>l) x ((h+2^l-1)>>l), tight rows. */
int svo_build_pyramid(svo_ctx* ctx, const uint8_t* img, int width, int height, int row_stride,
                      uint8_t* levels, size_t levels_bytes);

/* FeatureTracker::track_features (src/feature_tracker.cpp:18-67) as one call:
 * forward + backward LK and the survivor / parallax filter.
 * initial_xy[i] is the keyframe position of feature i (initial_features.at(id)).
 * Outputs: kept_xy (n x 2), kept_index (n; index into the input list, ascending),
 * *n_kept, *av_parallax (sum over kept / n, src/feature_tracker.cpp:59,63),
 * *percent_lost is left to the caller (needs |initial_features|, :64). */
int svo_track_features(svo_ctx* ctx, const uint8_t* prev, const uint8_t* next, int width,
                       int height, int row_stride, const float* xy, const float* initial_xy, int n,
                       float* kept_xy, int* kept_index, int* n_kept, float* av_parallax);

/* ------------------------------------------------------------------- a6 --
 * new-vs-tracked dedup loop (src/image_processor.cpp:113-128): keep detected[i]
 * iff no tracked[j] has sqrt(dx^2+dy^2) < min_distance. Stable order. */
int svo_dedup(svo_ctx* ctx, const float* detected_xy, int n_detected, const float* tracked_xy,
              int n_tracked, float min_distance, float* kept_xy, int* n_kept);

/* ------------------------------------------------------------------- a5 --
 * cv::solvePnPRansac(obj, img, K, 0, rvec, tvec, true, iters, reproj_err, conf, inliers)
 * (src/image_processor.cpp:76-80).  Deterministic restatement:
 * fixed-seed hypothesis sampling, Gauss-Newton minimal solves from the extrinsic
 * guess, inlier test err^2 <= reproj_err^2, refinement on the inliers.
 * rvec3/tvec3 are in/out doubles; inliers: n ints (ascending), *n_inliers. */
int svo_pnp_ransac(svo_ctx* ctx, const float* xyz, const float* xy, int n, float focal, float cx,
                   float cy, double* rvec3, double* tvec3, int iterations, float reproj_err,
                   double confidence, int* inliers, int* n_inliers);

/* ------------------------------------------------------------ a9,a10,a12,a13 --
 * Sliding-window bundle adjustment (src/bundle_adjuster.cpp:5-163).
 * The graph lives on the device; ids are assigned exactly as the reference does
 * (sequential in creation order, SURVEY C-3). */
typedef struct svo_ba svo_ba;

typedef struct svo_ba_options {
  int max_iterations;      /* Ceres default 50 */
  double max_time_s;       /* reference: 0.1 (src/bundle_adjuster.cpp:11); <=0 disables (parity runs) */
  double function_tolerance, gradient_tolerance, parameter_tolerance; /* 1e-6, 1e-10, 1e-8 */
  double initial_radius;   /* 1e4 */
  int max_features;        /* per keyframe; reference 400 (src/bundle_adjuster.hpp:75) */
  int accumulation;        /* how J^T J / the Schur products are summed: SVO_BA_ACC_* (default AUTO) */
} svo_ba_options;

/* AUTO: DETERMINISTIC (per-chunk partial sums in the declared summation order: bit-identical to the oracle) while the
 * partial store (wire elements x chunk groups x 16 bytes) fits 512 MB, else MFMA when eligible (<= 22 poses, one observation per (landmark, pose)), else ATOMICS. */
enum { SVO_BA_ACC_AUTO = 0, SVO_BA_ACC_DETERMINISTIC = 1, SVO_BA_ACC_ATOMICS = 2, SVO_BA_ACC_MFMA = 3 };

typedef struct svo_ba_summary {
  int iterations, successful_steps, termination; /* 0 conv, 1 no-conv(iter/time), 2 failure */
  double initial_cost, final_cost;
  double solve_ms;
} svo_ba_summary;

/* Sums `n_doubles` doubles at DEVICE pointer `dev_ptr` in place over all ranks (in-process emulation of the collective
 * for tests; production ranks hand over an RCCL communicator with svo_ba_set_comm instead). */
typedef int (*svo_allreduce_fn)(void* dev_ptr, size_t n_doubles, void* user);

/* ---- step control of ceres::Solve (src/bundle_adjuster.cpp:140) with pluggable passes ------------------------------
 * The LM loop itself (host/lm.cpp) is one piece of host code shared by every backend and every rank.  A backend
 * provides the two passes over the observations; payloads are host arrays ALREADY SUMMED over all ranks:
 *   payload1 (n*n + 3n + 2 doubles, n = 6 (K-1)): [S (n x n, full) | g_red | g_c | diag U | cost | sum g_p^2]
 *   payload2 (4 doubles): [candidate cost | landmark part of the model change | sum dp^2 | sum p^2]
 * linearize: pass A at the current point with `radius`; `first` != 0 fixes the landmarks' Jacobi scales.
 * step:      pass B at the current point: pose step dc (n) and candidate poses (7K) in, candidate landmarks formed,
 *            payload2 out.  The backend may also produce the NEXT iteration's payload1 in the same call, so that an LM
 *            iteration costs one host round trip (see host/lm.cpp):
 *              ctl->spec_radius > 0: pass A at the candidate with that radius in the same sweep; both payloads are
 *                summed by ONE collective;
 *              else ctl->chain != 0: once payload2 is summed, take Ceres' accept / radius decision where the sums live
 *                (svo_lm_decide, host/lm_decide.h, from ctl->cost, ctl->mcc, radius, ctl->decrease_factor) and run pass
 *                A for it: at the candidate with the new radius if accepted, at the current point with the reduced
 *                radius if not.
 *            *next_radius = the radius that pass A ran with (0: none was produced), *next_at_candidate = where.
 *            The step control re-derives the decision itself and uses payload1_next only if both agree.
 * accept:    the candidate becomes the current point.
 * Callbacks return 0 or an svo_status. */
typedef struct svo_lm_step_ctl {
  double cost, mcc, decrease_factor;
  double spec_radius;
  int chain;
} svo_lm_step_ctl;
typedef struct svo_lm_ops {
  void* user;
  int (*linearize)(void* user, double radius, int first, double* payload1);
  int (*step)(void* user, const double* dc, const double* cand_poses7, double radius, const svo_lm_step_ctl* ctl,
              double* payload2, double* payload1_next, double* next_radius, int* next_at_candidate);
  int (*accept)(void* user);
} svo_lm_ops;
typedef struct svo_lm_stats {
  int linearize_calls;   /* stand-alone pass-A calls (each one exchange) */
  int step_calls;        /* pass-B calls (each one exchange) */
  int speculations;      /* steps that also produced a linearisation for the next iteration (same sweep or chained) */
  int speculation_hits;  /* ... that the step control could use: the iteration cost exactly one host round trip */
  int single_exchange;   /* steps whose pass A rode in the SAME collective as payload2 (saturated-radius prediction) */
  int collectives;       /* all-reduce calls the solve issued (sharded runs; what N ranks would issue: also counted on one rank) */
  int device_control;    /* 1: the step control ran on the device (bulk / sharded path: no host work inside an LM iteration) */
  int fallbacks;         /* device-resident window solves that gave up and were re-run through the host-driven loop */
  double host_us;        /* host time spent inside the LM loop of the last solve (launch calls + waits that were not overlapped), us */
} svo_lm_stats;

void svo_ba_default_options(svo_ba_options* o);
/* The LM loop over caller-provided passes.  poses7: K x 7 current poses, updated in place on every accepted step
 * (pose 0 is constant, src/bundle_adjuster.cpp:130).  opt NULL = defaults.  stats may be NULL. */
int svo_lm_solve(int n_poses, double* poses7, const svo_lm_ops* ops, const svo_ba_options* opt,
                 svo_ba_summary* summary, svo_lm_stats* stats);
/* Ceres' accept / radius rule for one step (host/lm_decide.h; the kernels evaluate the same function): what a backend's
 * `step` uses for ctl->chain when its sums live on the host. */
int svo_lm_decide_step(double cost, double mcc, double radius, double decrease_factor, double cost_new,
                       double model_change_points, int* accept, double* next_radius);
int svo_ba_create(svo_ctx* ctx, svo_ba** out, int window_size, const svo_camera_info* cam,
                  const svo_ba_options* opt, int max_landmarks, int max_observations);
void svo_ba_destroy(svo_ba* ba);
/* forget all keyframes and landmarks, keep every buffer (a fresh BundleAdjuster without re-allocation). */
int svo_ba_reset(svo_ba* ba);
/* BundleAdjuster::add_keyframe (src/bundle_adjuster.cpp:60-135). pose7 from the
 * keyframe's (orientation, position) floats widened to double (:63-70).
 * tracked_ids/tracked_xy: n_tracked observations of existing landmarks;
 * new_xy/new_xyz: n_new fresh landmarks, truncated to max_features-n_tracked
 * (:85-90); new_ids receives the ids assigned, *n_new_out the surviving count. */
int svo_ba_add_keyframe(svo_ba* ba, const double* pose7, const int64_t* tracked_ids,
                        const float* tracked_xy, int n_tracked, const float* new_xy,
                        const float* new_xyz, int n_new, int64_t* new_ids, int* n_new_out);
/* BundleAdjuster::bundle_adjust (src/bundle_adjuster.cpp:137-157): no-op unless a
 * keyframe was added since the last solve. */
int svo_ba_solve(svo_ba* ba, svo_ba_summary* summary);
/* The dense SPD solve of the reduced camera system — what Ceres' DENSE_SCHUR does with Eigen's LLT inside
 * ceres::Solve (src/bundle_adjuster.cpp:156).  Host-only (the system is at most 378 x 378).  A: n x n
 * row-major, lower triangle read, overwritten by L; b: right-hand side, overwritten by the solution.
 * Declared operation order (see host/linalg.cpp): bit-identical to the plain left-looking loop.
 * Returns SVO_ERR_NUMERIC when A is not positive definite. */
int svo_cholesky_solve(double* A, double* b, int n);
/* The same solve by ONE workgroup on the GPU (csrc/lm_device.h): what the controller workgroup of the device-resident
 * solve runs between two passes, exposed for parity tests — bit-identical to svo_cholesky_solve.  Host pointers. */
int svo_cholesky_solve_dev(svo_ctx* ctx, double* A, double* b, int n);
/* pose of window slot k (0 = oldest, -1 = newest). */
int svo_ba_get_pose(svo_ba* ba, int k, double* pose7);
int svo_ba_window_count(svo_ba* ba);
/* BundleAdjuster::get_world_points (src/bundle_adjuster.cpp:159-163): double->float gather. */
int svo_ba_get_points(svo_ba* ba, const int64_t* ids, int n, float* xyz);

/* Bulk problem interface (synthetic BA of BASELINE config 4; also what a
 * sharded rank loads): poses K x 7 (pose 0 constant), points N x 3, observations
 * sorted by landmark: obs_pose/obs_point/obs_uv.  In a sharded run every rank
 * loads all poses and only its own landmarks; the payloads are summed over the ranks by
 * RCCL (svo_ba_set_comm) or by the `allreduce` callback (tests), once per LM iteration
 * when the speculative linearisation hits (host/lm.cpp), twice otherwise. */
int svo_ba_load_problem(svo_ba* ba, int n_poses, const double* poses7, int n_points,
                        const double* points3, int n_obs, const int32_t* obs_pose,
                        const int32_t* obs_point, const double* obs_uv);
int svo_ba_set_allreduce(svo_ba* ba, svo_allreduce_fn fn, void* user);
/* Sharded run over RCCL: `nccl_comm` is the rank's ncclComm_t (as void*).  The library calls
 * ncclAllReduce(sum, f64, in place) on the adjuster's own stream — one call per LM iteration when the speculative
 * linearisation hits (n*n + 3n + 2 + 8 doubles: 107 KB at K = 20), no host code in between.  NULL detaches. */
int svo_ba_set_comm(svo_ba* ba, void* nccl_comm);
/* RCCL communicator helpers for callers that have no other RCCL binding (C++ consumers such as the reference's
 * vo_node; bench.py).  They use the librccl already loaded in the process, else /opt/rocm/lib/librccl.so.1.
 * id128: 128-byte ncclUniqueId created on one rank and distributed by any out-of-band channel. */
int svo_rccl_unique_id(void* id128);
int svo_rccl_comm_create(void** nccl_comm, int n_ranks, int rank, const void* id128, int device);
int svo_rccl_comm_destroy(void* nccl_comm);
/* Where ceres::Solve's step control runs for window-sized, single-rank, deterministic solves (src/bundle_adjuster.cpp:140):
 * mode 1: on the device — the whole solve is ONE launch (csrc/ba.hip ba_lm_kernel), the host only waits for its completion
 * word; mode 0: on the host (host/lm.cpp), 1-3 launches per LM iteration; mode -1 (default): on the device while more
 * than two pipelines are inside svo_pipeline_process_batch* (pipeline groups always solve on the device).  Results are
 * bit-identical either way. */
int svo_ba_set_device_lm(svo_ba* ba, int mode);
/* Which form a device-resident window solve takes (both run src/bundle_adjuster.cpp:140's whole ceres::Solve on the device,
 * bit-identical to each other and to the host-driven loop):
 *   0 wide     ba_lm_kernel: one workgroup per two chunks of 64 observations (~47 for the reference's 5-keyframe window), replicated
 *              step control, lowest latency — a lone stereo stream (the reference's vo_node);
 *   1 compact  ba_lm_compact_kernel: ONE workgroup per solve, its wavefronts take the chunks in turn, step control once, nothing
 *              waits for another workgroup — 1/16 of the wide form's wavefronts and LDS for ~10x its latency (measured: it does not
 *              pay at 48-128 streams on one MI355X); the re-run of a wide solve that gave up, the overflow of the
 *              admission budget (SVO_BA_OVERFLOW=1); takes windows of up to 256 chunks (the wide form: 128);
 *  -1 default  SVO_BA_FORM=wide|compact if set, else wide. */
int svo_ba_set_solve_form(svo_ba* ba, int form);
/* Where the step control runs for BULK / SHARDED solves (hardware-order accumulation, svo_ba_load_problem +
 * svo_ba_solve_problem; the all-reduce of src/bundle_adjuster.cpp:140's normal equations over the ranks): mode 1 / -1 (default):
 * on the device — per LM iteration the host only enqueues [pass B, all-reduce, pass A, all-reduce, control kernel], a fixed
 * number of slots ahead of the control kernel's status records (csrc/ba.hip ba_bulk_control_kernel; reduced camera systems up
 * to n = 128); mode 0: host/lm.cpp drives every iteration (one D2H + host Cholesky + upload per iteration). */
int svo_ba_set_bulk_control(svo_ba* ba, int mode);
/* counters of the last svo_ba_solve / svo_ba_solve_problem */
int svo_ba_last_stats(svo_ba* ba, svo_lm_stats* stats);
/* Chunks of 64 observation slots that every wavefront of this adjuster's WIDE device-resident solves takes in turn: k = 1 ..
 * svo_ba_wave_chunks_limit() (fewer workgroups per solve, a longer LM chain; the bits do not depend on k), 0 (default): the
 * process default (3, SVO_BA_WAVE_CHUNKS), which the admission raises for a solve that its budget of co-resident workgroups
 * refuses at the default. */
int svo_ba_wave_chunks_limit(void);
int svo_ba_set_wave_chunks(svo_ba* ba, int k);
/* Device-resident solves this adjuster has launched since it was created: counts[0] in the compact form (one workgroup),
 * counts[k] in the wide form at k chunks per wavefront; entries beyond the limit are 0.  gave_up (may be null): how many of
 * them gave up within their bounded waits and were run again (compact form, else host-driven) — such a solve counts in both
 * forms.  counts[svo_ba_wave_chunks_limit() + 1], where n reaches that far: continuation launches of the finished wide solves
 * that stepped aside (svo_ba_set_yield_iterations); such a solve counts once, at the k of its first launch. */
int svo_ba_solve_forms(svo_ba* ba, long* counts, int n, long* gave_up);
/* LM iterations a WIDE device-resident solve of this adjuster (several chunks per wavefront) runs in one launch before it steps
 * aside: its state stays on the device and its next launch continues it, with the same bits as the uninterrupted solve.  A launch
 * shared by several solves lasts as long as its longest one; with n > 0 none outlasts n iterations.  0: never; -1 (default): what
 * SVO_BA_YIELD_ITERS says, else never.  svo_ba_solve_problem(s) and svo_ba_solve launch a solve again until it is done.  Solves
 * with a wall-clock cap (max_time_s > 0) never step aside.  Not while a solve of the adjuster is in flight or waits to continue. */
int svo_ba_set_yield_iterations(svo_ba* ba, int n);
int svo_ba_solve_problem(svo_ba* ba, svo_ba_summary* summary);
/* svo_ba_solve_problem for the loaded problems of n adjusters (of one context, n <= 64) at once: those that are eligible for the
 * wide device-resident form and admitted leave as ONE launch — as the lanes of a pipeline group do —, the others are solved one
 * by one.  summaries: n entries or null.  Returns how many shared the launch, or a negative error code. */
int svo_ba_solve_problems(svo_ba** bas, int n, svo_ba_summary* summaries);
int svo_ba_read_problem(svo_ba* ba, double* poses7, double* points3);

/* ---------------------------------------------------------------- pipeline --
 * ImageProcessor::process + BundleAdjuster::bundle_adjust for a batch of
 * consecutive frames already resident in HBM (src/image_processor.cpp:18-163,
 * driver loop src/vo_node.cpp:141-148).  Stateless stages (a1, pyramids) are
 * batched over the frames; the sequential chain runs per frame.  Results are
 * identical to frame-by-frame processing. */
typedef struct svo_pipeline svo_pipeline;
typedef struct svo_pipeline_params {
  svo_camera_info cam;
  int width, height;
  int max_corners;            /* 300 */
  double quality;             /* 0.1 */
  float min_feature_distance; /* 30 (src/vo_node.cpp:34) */
  float parallax_thresh;      /* 20 (src/vo_node.cpp:33) */
  int window_size;            /* 5  (src/vo_node.cpp:36) */
  int max_features;           /* 400 */
  int ba_max_iterations;      /* 50 */
  double ba_max_time_s;       /* 0.1; <=0 disables */
} svo_pipeline_params;

typedef struct svo_frame_result {
  int n_detected, n_tracked, n_inliers, n_new;
  int is_keyframe;       /* 1 if this frame became a keyframe */
  float av_parallax, percent_lost;
  double pose7[7];       /* last keyframe pose (world wrt camera) after bundle_adjust */
  int ba_iterations;
} svo_frame_result;

void svo_pipeline_default_params(svo_pipeline_params* p);
int svo_pipeline_create(svo_ctx* ctx, svo_pipeline** out, const svo_pipeline_params* p);
void svo_pipeline_destroy(svo_pipeline* p);
int svo_pipeline_reset(svo_pipeline* p);
/* left/right: batch images, tight rows (row stride = width), image stride = width*height. */
int svo_pipeline_process_batch_dev(svo_pipeline* p, const uint8_t* left, const uint8_t* right,
                                   int batch, svo_frame_result* results);
int svo_pipeline_process_batch(svo_pipeline* p, const uint8_t* left, const uint8_t* right,
                               int batch, svo_frame_result* results);
/* Raw input (coefficients of src/camera_info.hpp:10-14, per eye): builds both tables for the pipeline's camera and size,
 * uploads them and allocates the rectified workspace (max_batch x 2 x width x height bytes) once; nothing is allocated per
 * frame afterwards.  svo_pipeline_process_batch_dev / _batch then take left/right as RAW images: one remap launch in
 * front, every stage reads the rectified copy.  NULL, NULL turns it off and frees both.  Never called: nothing changes. */
int svo_pipeline_set_rectification(svo_pipeline* p, const svo_rectify_eye* left, const svo_rectify_eye* right);
/* Dense depth cloud per keyframe (src/image_processor.cpp:173-207 over the whole image; the reference's own landmark publisher
 * is commented out at src/vo_node.cpp:133).  params != NULL allocates everything once (maps, points, counts for
 * max_keyframes_per_call pairs; 0 = the context's max_batch; params->max_points <= 0 = width*height); afterwards every
 * svo_pipeline_process_batch[_dev] call, once its last frame is finished, runs ONE batched dense launch and ONE cloud launch
 * sequence over exactly the pairs of this call's frames with results[i].is_keyframe (the rectified copies when rectification
 * is set), StereoBM(48, 21) as the pipeline itself.  Clouds are in the keyframe's CAMERA frame (pose16 = identity): bundle
 * adjustment keeps moving keyframe poses, so the caller places a cloud with the keyframe's refined pose7.  The frame loop, the
 * stage order and svo_frame_result are untouched.  More keyframes in a call than the bound: the frame results are complete,
 * no cloud is produced and the call returns SVO_ERR_CAPACITY.  NULL turns it off and frees everything.  Never called: no
 * launch, no allocation, nothing changes. */
int svo_pipeline_set_keyframe_clouds(svo_pipeline* p, const svo_cloud_params* params, int max_keyframes_per_call);
/* Speckle filter of the keyframe maps (above): with params != NULL every process call runs the filter's launches between the
 * dense launch and the cloud launches, on the same stream, so the clouds are those of the filtered maps.  Keyframe clouds must be
 * on already (SVO_ERR_INVALID otherwise); the work space for max_keyframes_per_call maps is allocated once here.  NULL turns the
 * filter off and frees it; so does turning the clouds off.  New cloud parameters keep the filter.  Only the dense maps are
 * filtered: the sparse StereoBM that feeds landmarks, svo_frame_result and the tracked set do not change.  Never called: no
 * launch, no allocation, nothing changes. */
int svo_pipeline_set_keyframe_speckle_filter(svo_pipeline* p, const svo_speckle_params* params);
/* Left-right check of the keyframe maps (above, "left-right check"): with params != NULL every process call launches the cost
 * form of the dense kernel, then the check, then the speckle filter if that is on, then the clouds, on the same stream (the order
 * of StereoBM::compute).  The two filters are independent switches.  Keyframe clouds must be on already (SVO_ERR_INVALID
 * otherwise); the cost maps for max_keyframes_per_call maps (2 bytes per pixel) are allocated once here.  NULL turns the check off
 * and frees them; so does turning the clouds off.  New cloud parameters keep the check.  Only the dense maps are checked: the
 * sparse StereoBM that feeds landmarks, svo_frame_result and the tracked set do not change.  Never called: no launch, no
 * allocation, nothing changes, and the dense launch is the plain kernel. */
int svo_pipeline_set_keyframe_lr_check(svo_pipeline* p, const svo_lr_check_params* params);
/* Semi-global matching for the keyframe maps (above, "semi-global matching"): with params != NULL every process call runs the
 * matching sequence of svo_stereo_sgm_batch_dev (48, 21) instead of the dense launch, SVO_SGM_KEYFRAME_SUB_BATCH keyframes at a
 * time, then the left-right check (fed by the cost form of item 4) and the speckle filter if those are on, then the clouds, on
 * the same stream.  The three switches are independent.  Keyframe clouds must be on already (SVO_ERR_INVALID otherwise); the
 * work space for SVO_SGM_KEYFRAME_SUB_BATCH pairs is allocated once here, so max_keyframes_per_call does not multiply it.  NULL
 * returns to block matching and frees it; so does turning the clouds off.  New cloud parameters keep the switch.  Only the
 * dense maps change: the sparse StereoBM that feeds landmarks, svo_frame_result and the tracked set do not.  Never called: no
 * launch, no allocation, nothing changes. */
int svo_pipeline_set_keyframe_sgm(svo_pipeline* p, const svo_sgm_params* params);
/* One entry per keyframe of the last process call, in frame order (src/image_processor.cpp:173-207 per entry). */
typedef struct svo_keyframe_cloud {
  int frame;                  /* index in the call */
  int lane;                   /* 0 for an svo_pipeline */
  int n_total, n_stored;
  const svo_cloud_point* dev; /* DEVICE pointer to n_stored records */
} svo_keyframe_cloud;
/* The table of the last process call (src/image_processor.cpp:173-207); valid until the next process call. */
int svo_pipeline_keyframe_clouds(svo_pipeline* p, int* n, const svo_keyframe_cloud** table);
/* Entry i's points to HOST memory (src/image_processor.cpp:173-207): min(n_stored, capacity) records, synchronous. */
int svo_pipeline_copy_keyframe_cloud(svo_pipeline* p, int i, svo_cloud_point* host, int capacity);
/* Entry i's disparity map as its cloud was formed from it (after whichever of the left-right check and the speckle filter are
 * on): *dev is a DEVICE pointer to a tight width x height CV_16S map, valid until the next process call like the table.  What
 * svo_voxel_map_carve_pose7_dev takes; svo_keyframe_cloud itself is unchanged. */
int svo_pipeline_keyframe_disparity(svo_pipeline* p, int i, const int16_t** dev);
/* The same map to HOST memory (width * height int16), synchronous: what a caller keeps to carve later, and what the tests restate. */
int svo_pipeline_copy_keyframe_disparity(svo_pipeline* p, int i, int16_t* host);
/* Feature-set taps for parity tests: ids + positions the tracker holds after the last frame. */
int svo_pipeline_get_tracked(svo_pipeline* p, int64_t* ids, float* xy, int capacity, int* n);

/* ------------------------------------------------------------ pipeline group --
 * The same per-frame path (ImageProcessor::process + BundleAdjuster::bundle_adjust, src/image_processor.cpp:18-163,
 * src/vo_node.cpp:141-148) for n_lanes independent stereo streams behind ONE caller thread: each lane keeps its own
 * tracker, graph and poses exactly as an svo_pipeline does, every stage that several lanes reach together is ONE kernel
 * launch (blockIdx.y = lane) and their bundle adjustments are ONE device-resident solve launch; lanes never wait for
 * each other.  Lane results are bit-identical to n_lanes separate svo_pipeline objects.  The context's
 * svo_limits.max_batch bounds n_lanes x frames per call; 1 <= n_lanes <= 64.  (No reference counterpart: the reference is one stream in one
 * process; this is how one GPU serves many of them — and what a rank of the multi-GPU bench runs.) */
typedef struct svo_pipeline_group svo_pipeline_group;
int svo_pipeline_group_create(svo_ctx* ctx, svo_pipeline_group** out, const svo_pipeline_params* p, int n_lanes);
void svo_pipeline_group_destroy(svo_pipeline_group* g);
int svo_pipeline_group_reset(svo_pipeline_group* g);
int svo_pipeline_group_lanes(const svo_pipeline_group* g);
/* left/right: DEVICE pointers; lane l's `batch` images (tight rows, image stride = width*height) start lane_stride bytes
 * after lane l-1's.  results: n_lanes x batch, lane-major. */
int svo_pipeline_group_process_batch_dev(svo_pipeline_group* g, const uint8_t* left, const uint8_t* right, size_t lane_stride,
                                         int batch, svo_frame_result* results);
/* Host-pointer / streaming entry.  The reference hands over HOST images frame by frame (cv::Mat copies made in the image
 * callback, src/vo_node.cpp:70-73, consumed at :141-143): a group takes them through TWO pinned staging slots it owns.
 *   svo_pipeline_group_staging   the slot's buffers: n_lanes x max_batch x height x width bytes each, lane_stride =
 *                                max_batch x width x height.  The caller writes the next batch there in place (the
 *                                callback's copy lands where the DMA engine reads it: no second host copy);
 *   svo_pipeline_group_upload    starts the H2D copy of the slot's first `batch` frames per lane on the group's copy stream
 *                                and returns at once: the upload of batch b+1 overlaps the processing of batch b;
 *   svo_pipeline_group_process_uploaded  waits for the slot's upload, then processes it exactly as
 *                                svo_pipeline_group_process_batch_dev does (bit-identical results);
 *   svo_pipeline_group_process_batch     convenience, nothing overlapped: caller-owned host images are copied into slot 0,
 *                                uploaded and processed (what ImageProcessor::process(const StereoPair&) does, for every lane).
 * Streaming loop: fill(0); upload(0); for b: { fill((b+1)&1); upload((b+1)&1); process_uploaded(b&1); }. */
int svo_pipeline_group_staging(svo_pipeline_group* g, int slot, uint8_t** left, uint8_t** right, size_t* lane_stride);
int svo_pipeline_group_upload(svo_pipeline_group* g, int slot, int batch);
int svo_pipeline_group_process_uploaded(svo_pipeline_group* g, int slot, svo_frame_result* results);
int svo_pipeline_group_process_batch(svo_pipeline_group* g, const uint8_t* left, const uint8_t* right, size_t lane_stride,
                                     int batch, svo_frame_result* results);
/* svo_pipeline_set_rectification for lane `lane` (-1: every lane; coefficients of src/camera_info.hpp:10-14 per eye).  Lanes
 * may have different cameras; lanes set from the same pair of models share one copy of the tables in HBM.  Covers
 * svo_pipeline_group_process_batch_dev, _process_uploaded and _process_batch alike: ONE remap launch per call for all
 * rectified lanes, issued on the processing side (after the slot's upload has been waited for, so the streaming loop's
 * overlap of upload and processing is untouched); lanes without a model are neither remapped nor copied. */
int svo_pipeline_group_set_rectification(svo_pipeline_group* g, int lane, const svo_rectify_eye* left, const svo_rectify_eye* right);
/* svo_pipeline_set_keyframe_clouds for lane `lane` (-1: every lane; src/image_processor.cpp:173-207 per keyframe).  After the
 * call's event loop has drained: ONE dense launch and ONE cloud launch sequence for all (lane, frame) keyframes of the call of
 * the lanes that have clouds on; lanes without cost nothing.  Covers _process_batch_dev, _process_uploaded and _process_batch.
 * The lanes that have clouds on share one set of parameters and one bound (a differing set while another lane is on:
 * SVO_ERR_INVALID); max_keyframes_per_call counts all lanes together, 0 = the context's max_batch.  The table is ordered by
 * lane, then frame. */
int svo_pipeline_group_set_keyframe_clouds(svo_pipeline_group* g, int lane, const svo_cloud_params* params, int max_keyframes_per_call);
/* svo_pipeline_set_keyframe_speckle_filter for the group: the lanes that have clouds on share one set of buffers and one cloud
 * parameter set, so the filter is group-wide as well.  Clouds must be on for at least one lane. */
int svo_pipeline_group_set_keyframe_speckle_filter(svo_pipeline_group* g, const svo_speckle_params* params);
/* svo_pipeline_set_keyframe_lr_check for the group, group-wide like the speckle filter.  Clouds must be on for at least one lane. */
int svo_pipeline_group_set_keyframe_lr_check(svo_pipeline_group* g, const svo_lr_check_params* params);
/* svo_pipeline_set_keyframe_sgm for the group, group-wide like the two filters.  Clouds must be on for at least one lane. */
int svo_pipeline_group_set_keyframe_sgm(svo_pipeline_group* g, const svo_sgm_params* params);
int svo_pipeline_group_keyframe_clouds(svo_pipeline_group* g, int* n, const svo_keyframe_cloud** table);
int svo_pipeline_group_copy_keyframe_cloud(svo_pipeline_group* g, int i, svo_cloud_point* host, int capacity);
/* svo_pipeline_keyframe_disparity for entry i of the group's table. */
int svo_pipeline_group_keyframe_disparity(svo_pipeline_group* g, int i, const int16_t** dev);
int svo_pipeline_group_copy_keyframe_disparity(svo_pipeline_group* g, int i, int16_t* host);
int svo_pipeline_group_get_tracked(svo_pipeline_group* g, int lane, int64_t* ids, float* xy, int capacity, int* n);
/* Launch statistics of the last process_batch call, by stage: 0 track (LK + compaction), 1 PnP-RANSAC (hypotheses, bookkeeping and
 * refinement in one launch), 3 dedup / stereo + triangulation, 4 bundle-adjustment solves, 5 corner detection + pyramids;
 * launches6[i] launches carried lanes6[i] lane-stages in total.  Slot 2 (round 5) is the driving thread instead: launches6[2] = microseconds of
 * its loop passes that did something, lanes6[2] = microseconds of the call's main loop. */
int svo_pipeline_group_last_stats(const svo_pipeline_group* g, long* launches6, long* lanes6);
/* Algorithmic work (SURVEY 8(d) per-iteration figures: 466 flops per observation + 50 + 144 L + 216 L (L + 1) / 2 per landmark;
 * 24 B per observation + 48 B per landmark + 56 B per pose) of the bundle adjustments all lanes have finished since the last
 * reset: out4 = [f64 flops, bytes, solves, LM iterations].  Measurement aid (bench.py's roofline of the solve kernel). */
int svo_pipeline_group_solve_work(svo_pipeline_group* g, double* out4, int reset);
/* svo_ba_solve_forms summed over the lanes' adjusters: "compact solves" and "wide solves at k" of a profile. */
int svo_pipeline_group_solve_forms(svo_pipeline_group* g, long* counts, int n, long* gave_up);
/* svo_ba_set_yield_iterations for every lane's adjuster (n >= 0): a solve that stepped aside rides the group's next wide launch,
 * in front of the solves that have never run.  A group starts with SVO_BA_YIELD_ITERS, else with the library's default. */
int svo_pipeline_group_set_solve_yield(svo_pipeline_group* g, int n);

/* FeatureTracker::draw_track + get_drawing (src/feature_tracker.cpp:74-91; used by src/vo_node.cpp:137,188):
 * the keyframe image as RGB (3 bytes per pixel, width*height*3 output) with one green arrow of thickness 4 per feature
 * from its keyframe position to its current position.  Host-side visualisation with this repository's own rasteriser
 * (same picture as cv::arrowedLine, not pixel-identical). */
int svo_draw_track(const uint8_t* gray, int width, int height, int row_stride, const float* from_xy,
                   const float* to_xy, int n, uint8_t* rgb);
/* The same for a pipeline's tracker: `keyframe_gray` is the host copy of the image the tracker was (re)initialised
 * on (the reference keeps a clone, :14); arrows come from the tracker's initial / current feature positions. */
int svo_pipeline_draw_track(svo_pipeline* p, const uint8_t* keyframe_gray, int row_stride, uint8_t* rgb);

/* ------------------------------------------------------------- synthetic data --
 * Deterministic KITTI-shaped stereo stream: integer PRNG, ray-cast
 * textured billboards; host buffers; bit-identical on every host. Not part of the
 * reference; test/bench input only. */
typedef struct svo_synth_params {
  uint64_t seed;
  int width, height;
  double focal, cx, cy, baseline;
  double step_z, step_x, yaw_per_frame; /* camera motion per frame */
  int n_billboards;
} svo_synth_params;
void svo_synth_default_params(svo_synth_params* p, int width, int height);
int svo_synth_render(const svo_synth_params* p, int frame, uint8_t* left, uint8_t* right);
/* ground-truth camera-in-world pose of `frame` as 3x4 row-major [R|t] (KITTI poses row format,
 * src/kitti_node.cpp:47-50). */
int svo_synth_pose(const svo_synth_params* p, int frame, double* rt12);

/* ------------------------------------------------ dataset ingestion, driver, ATE --
 * KITTI odometry layout read by the reference's kitti_node (src/kitti_node.cpp:37-68): images
 * <data_path><SS>/image_0|image_1/%06d.png (8-bit gray), poses <data_path>data_odometry_poses/dataset/poses/SS.txt
 * (12 doubles per row, row-major 3x4 [R|t], camera in world).  PNG (zlib only) and PGM are decoded. */
int svo_image_read_gray(const char* path, uint8_t* buf, size_t capacity, int* width, int* height);
int svo_kitti_read_poses(const char* poses_file, double* rt12, int capacity_frames, int* n_frames);
/* RMSE of positions after the best rigid (with_scale: similarity) alignment est -> gt. */
int svo_ate_rmse(const double* est_xyz, const double* gt_xyz, int n, int with_scale, double* rmse);
typedef struct svo_run_stats {
  int frames, keyframes;
  double ate_rmse; /* vs the poses file, evaluated at keyframes, rigid alignment; -1 without ground truth */
  double seconds;
} svo_run_stats;
/* Non-ROS driver with vo_node's loop semantics (src/vo_node.cpp:141-150): process + bundle_adjust per frame,
 * one camera-in-world pose per processed frame written to traj_rt12 (max_frames x 12, may be NULL). */
int svo_kitti_run(svo_ctx* ctx, const svo_pipeline_params* params, const char* data_path, int sequence,
                  int max_frames, double* traj_rt12, svo_run_stats* stats);

#ifdef __cplusplus
}
#endif
#endif /* SVO_H_ */
