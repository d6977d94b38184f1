// Internal device-pointer entry points shared between the C-ABI wrappers and the in-library
// pipeline (host/pipeline.cpp).  All asynchronous on ctx->stream.  Counts that are produced on the
// device stay on the device (`const int* n_dev`) so stages chain without host round trips;
// `n_max` bounds the launch.
#ifndef SVO_KERNELS_H_
#define SVO_KERNELS_H_
#include "common.h"

struct SvoMat4 { float m[16]; };

// a8: M = float(pose * Q) formed on the host in the reference's order (src/image_processor.cpp:183-189,202).
SvoMat4 svo_k_reprojection_matrix(const float* pose16, float focal, float cx, float cy, float baseline);
SvoMat4 svo_k_reprojection_q(float focal, float cx, float cy, float baseline);  // the Q of that product alone (pose = identity is NOT applied)
int svo_k_triangulate(svo_ctx* ctx, const float* xy, const float* disp, const int* n_dev, int n_max,
                      const SvoMat4& M, float* kept_xy, float* xyz, int* kept_index, int* n_kept,
                      const SvoPublish* pub = nullptr);
// a7 (sparse) + a8 in one launch: disparities at the n features, triangulation / compaction by the last workgroup; the
// outputs may be pinned host memory, `*pub_out` is the completion word to wait for (svo_wait_word)
int svo_k_stereo_triangulate(svo_ctx* ctx, const uint8_t* left, const uint8_t* right, int width, int height, int row_stride,
                             int num_disparities, int block_size, const float* xy, const int* n_dev, int n_max, float* disp,
                             const SvoMat4& M, float* kept_xy, float* xyz, int* kept_index, int* n_kept, int word, SvoPublish* pub_out);
// a6
int svo_k_dedup(svo_ctx* ctx, const float* det_xy, const int* n_det_dev, int n_det_max, const float* trk_xy,
                const int* n_trk_dev, int n_trk_max, float min_distance, float* kept_xy, int* n_kept);
// a3: pyramid of `batch` images. levels buffer: per image svo_k_pyramid_bytes(w,h) bytes, level 0 first.
size_t svo_k_pyramid_bytes(int w, int h);
int svo_k_build_pyramid(svo_ctx* ctx, const uint8_t* imgs, int batch, int w, int h, int row_stride,
                        size_t image_stride, uint8_t* pyr, size_t pyr_stride, bool level0_in_place = false);
int svo_k_pyramid_level0(svo_ctx* ctx, const uint8_t* imgs, int batch, int w, int h, int row_stride, size_t image_stride, uint8_t* pyr,
                         size_t pyr_stride, hipStream_t st);
// forward+backward LK and the survivor filter of FeatureTracker::track_features.
// optional extras of the compaction step: per-feature state carried along with the kept features, and pinned
// host words that receive (n_kept, av_parallax) directly
struct SvoTrackCarry {
  const float* init_src = nullptr; const long long* ids_src = nullptr;
  float* init_dst = nullptr; long long* ids_dst = nullptr;
  int* host_n = nullptr; float* host_av = nullptr;           // pinned words for (n_kept, av_parallax)
  float* host_xy = nullptr; long long* host_ids = nullptr;   // pinned mirrors of the kept features / ids
  SvoPublish pub;                                            // completion word published after all of the above
};
int svo_k_track(svo_ctx* ctx, const uint8_t* pyr_prev, const uint8_t* pyr_next, int w, int h, const float* xy,
                const float* initial_xy, const int* n_dev, int n_max, float* fwd_xy, uint8_t* keep_flag,
                float* parallax, float* kept_xy, int* kept_index, int* n_kept, float* av_parallax,
                const SvoTrackCarry* carry = nullptr);
int svo_k_lk(svo_ctx* ctx, const uint8_t* pyr_prev, const uint8_t* pyr_next, int w, int h, const float* xy,
             int n, float* out_xy, uint8_t* status);
// gathers used by the tracker / pipeline: dst[i] = src[idx[i]] for i < n (n on the device or host)
int svo_k_gather_track(svo_ctx* ctx, const int* idx, const int* n_dev, int n_max, const float* init_src,
                       const long long* ids_src, float* init_dst, long long* ids_dst);
// tracker (re)initialisation from pinned host arrays: d_xy = d_init = h_xy, d_ids = h_ids (one launch, no H2D blits)
int svo_k_tracker_init(svo_ctx* ctx, const float* h_xy, const float* h_init, const long long* h_ids, int n, float* d_xy, float* d_init,
                       long long* d_ids, const SvoPublish* pub);
int svo_k_gather_xy_ids(svo_ctx* ctx, const int* idx, int n, const float* xy_src, const long long* ids_src,
                        float* xy_dst, long long* ids_dst);
// a5 (device-pointer form)
int svo_k_pnp(svo_ctx* ctx, SvoScratch& s, const float* d_xyz, const float* d_xy, int n, float focal, float cx, float cy,
              double* rvec3, double* tvec3, int iterations, float reproj_err, double confidence, int* d_inliers,
              int* n_inliers, int* h_inliers = nullptr /* pinned: also receives the inlier list */,
              float* d_inlier_xy = nullptr /* device: xy of the inliers, in list order (the dedup stage's input) */);
// rectification (csrc/rectify.hip, host/rectify.cpp): ONE launch warps every image of a call.  Image z of the launch is
// (active lane k, frame f, eye e) = (z / eyes / frames, z / eyes % frames, z % eyes); active lane k is lane `lane[k]` of the
// caller's layout and reads the tables map[k][e] (int32 records, dx in the low half, tight rows of `width`).
constexpr int SVO_RECT_MAX_LANES = 64;
constexpr int SVO_RECT_SENTINEL = (int)0x80008000u;  // (dx, dy) = (-32768, -32768): no source
struct SvoRectifyArgs {
  const uint8_t* src[2];  // per eye: lane 0's first raw image
  uint8_t* dst[2];        // per eye: lane 0's first rectified image (tight rows)
  size_t src_lane_stride, src_image_stride, dst_lane_stride, dst_image_stride;
  int src_row_stride, width, height, frames, eyes, n_active;
  const int* map[SVO_RECT_MAX_LANES][2];
  unsigned char lane[SVO_RECT_MAX_LANES];
};
int svo_k_rectify_remap(svo_ctx* ctx, const SvoRectifyArgs& a, hipStream_t st);
// The tables of one stereo camera (or of one eye: right == nullptr) in HBM, shared by every lane set from the same models.
struct SvoRectModel {
  svo_rectify_eye eye[2];
  int* d_map[2] = {nullptr, nullptr};
  int refs = 0;
};
int svo_rect_model_create(svo_ctx* ctx, const svo_rectify_eye* left, const svo_rectify_eye* right, const svo_camera_info* cam,
                          int width, int height, SvoRectModel** out);
void svo_rect_model_destroy(SvoRectModel* m);
// dense depth clouds (csrc/dense.hip).  Where pair z of a batched launch lives: z * image_stride after left / right, or tab[z]
// (a DEVICE table) when the pairs are scattered (the keyframes of a call).
struct SvoCloudPair { const uint8_t* left; const uint8_t* right; };
struct SvoDensePairs {
  const uint8_t* left;
  const uint8_t* right;
  size_t image_stride;
  const SvoCloudPair* tab;
};
// cost16 != null: the cost form of the kernel, which also writes the winner's SAD per pixel (0xFFFF where the map is FILTERED)
int svo_k_stereo_dense_batch(svo_ctx* ctx, const SvoDensePairs& src, int batch, int W, int H, int stride, int ndisp, int block, int16_t* disp16,
                             uint16_t* cost16 = nullptr);
int svo_k_cloud(svo_ctx* ctx, const int16_t* disp16, const SvoDensePairs& src, int batch, int W, int H, int stride, const svo_camera_info* cam,
                const float* pose16, const svo_cloud_params* prm, svo_cloud_point* points, int* counts, int* seg);  // seg: cloud_chunks ints per image
// The argument rules of everything from here to the keyframe clouds, their messages, the buffer sizes and the launch geometry are
// host/dense_args.h (plain C++, walked on a CPU by tests/sanitize/dense_args_test.cpp); the svo_k_* below trust their arguments.
// speckle filter (csrc/speckle.hip): the four launches over `batch` tight maps, in place; workspace: speckle_workspace_bytes;
// n_removed: batch device ints or null.  max_size == 0 launches nothing.
int svo_k_speckle(svo_ctx* ctx, int16_t* disp16, int batch, int W, int H, const svo_speckle_params* prm, void* workspace, int* n_removed);
// left-right check (csrc/lr_check.hip): one launch over `batch` tight maps, in place, from the winner's SAD per pixel;
// n_removed: batch device ints or null.
int svo_k_lr_check(svo_ctx* ctx, int16_t* disp16, const uint16_t* cost16, int batch, int W, int H, const svo_lr_check_params* prm, int* n_removed);
// semi-global matching (csrc/sgm.hip): fill, cost volume and the four path launches over `batch` pairs as ONE profile bracket;
// workspace: sgm_workspace_bytes; cost16 may be null.
int svo_k_stereo_sgm(svo_ctx* ctx, const SvoDensePairs& src, int batch, int W, int H, int stride, int ndisp, int block,
                     const svo_sgm_params* prm, void* workspace, int16_t* disp16, uint16_t* cost16);
// The keyframe clouds of one pipeline or one group (host/keyframe_clouds.cpp): every buffer allocated once by create; run() = one
// dense launch (with svo_kfc_set_sgm: the semi-global matching sequence per sub-batch of SVO_SGM_KEYFRAME_SUB_BATCH pairs instead)
// + (with svo_kfc_set_lr_check) the left-right check + (with svo_kfc_set_speckle) the speckle filter's launches + one cloud launch
// sequence over the given pairs on the context's stream, then waits and fills the table.
struct SvoKfClouds;
int svo_kfc_create(svo_ctx* ctx, const svo_cloud_params* params, int W, int H, int max_keyframes, SvoKfClouds** out);
void svo_kfc_destroy(SvoKfClouds* k);
// *slot (may be null) gives way to a fresh object for these parameters, and the switches that were on are carried over.  On any
// failure *slot stays as it is and the fresh object is destroyed.
int svo_kfc_replace(svo_ctx* ctx, SvoKfClouds** slot, const svo_cloud_params* params, int W, int H, int max_keyframes);
const svo_cloud_params* svo_kfc_params(const SvoKfClouds* k);  // as resolved by create (max_points > 0)
int svo_kfc_max_keyframes(const SvoKfClouds* k);
void svo_kfc_clear(SvoKfClouds* k);
// The three switches, one pattern: a non-null call checks the parameters, allocates the stage's buffer if this is the first, and
// switches the stage on; a null call waits for the stream, frees the buffer and switches it off.
//   speckle : the filter between the matcher and the clouds; its work space for max_keyframes maps
//   lr_check: the check between the matcher and the speckle filter; the cost maps for max_keyframes maps.  While it is on, run()
//             launches the cost form of the dense kernel (or of the semi-global matching)
//   sgm     : semi-global matching instead of the dense launch; the workspace for SVO_SGM_KEYFRAME_SUB_BATCH pairs
int svo_kfc_set_speckle(SvoKfClouds* k, const svo_speckle_params* prm);
int svo_kfc_set_lr_check(SvoKfClouds* k, const svo_lr_check_params* prm);
int svo_kfc_set_sgm(SvoKfClouds* k, const svo_sgm_params* prm);
int svo_kfc_run(SvoKfClouds* k, const svo_camera_info* cam, const SvoCloudPair* pairs, const int* frame, const int* lane, int n);
int svo_kfc_table(SvoKfClouds* k, int* n, const svo_keyframe_cloud** table);
int svo_kfc_copy(SvoKfClouds* k, int i, svo_cloud_point* host, int capacity);
int svo_kfc_disparity(SvoKfClouds* k, int i, const int16_t** dev);  // entry i's map as its cloud was formed from it
int svo_kfc_copy_disparity(SvoKfClouds* k, int i, int16_t* host);   // the same, W * H values to the host, synchronous
// What csrc/voxel_align.hip reads a voxel map through (csrc/voxel.hip owns the map): the table's five arrays, read only.
struct SvoVoxelView {
  svo_ctx* ctx;
  const unsigned long long *keys, *ci, *sx, *sy, *sz;
  unsigned long long mask;  // cap - 1
  float voxel_size, max_depth;
};
SvoVoxelView svo_voxel_map_view(const svo_voxel_map* m);  // m is not null
const char* svo_rectify_error_text();  // of the calling thread's last context-free rectification call ("" if none failed)
#endif
