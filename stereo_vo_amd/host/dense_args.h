// The dense keyframe chain's host logic that needs no GPU (include/svo.h, "dense depth clouds" .. "semi-global matching"; DESIGN
// §7b-§7e): the constants the host and the kernels share, the argument rules of the StereoBM, cloud, speckle, left-right and SGM
// entries, their buffer sizes and launch geometry, and the sizes of a pipeline's keyframe clouds.  A refusal is SVO_ERR_INVALID
// with *err set to the message; the .hip files and host/keyframe_clouds.cpp store it in the context (SVO_ARGS_CHECK) and keep no
// second copy of anything here.  tests/sanitize/dense_args_test.cpp walks every rule at its boundary on a CPU.
#ifndef SVO_DENSE_ARGS_H_
#define SVO_DENSE_ARGS_H_
#include <stddef.h>
#include <stdint.h>

#include "host_call.h"
#include "svo.h"

#define DENSE_REFUSE(cond, msg) do { if (!(cond)) { *err = (msg); return SVO_ERR_INVALID; } } while (0)

inline int dense_div_up(int a, int b) { return (a + b - 1) / b; }

// ----------------------------------------------------------------------------- what the host and the kernels share
constexpr int MAX_NDISP = 64, MAX_BLOCK = 21;
// Dense kernels: workgroup = 64 columns x 8 rows of output (see stereo_dense_kernel).
constexpr int DT_W = 64, DT_H = 8, DT_PIX = DT_W * DT_H;
constexpr int DT_TH = DT_H + MAX_BLOCK - 1;         // 28 tile rows
constexpr int DT_TWL = DT_W + MAX_BLOCK - 1;        // 84 left tile columns
constexpr int DT_TWR = DT_TWL + MAX_NDISP;          // right tile columns
constexpr int DT_SLOTS = 3;                         // disparity slots per pass
constexpr int CL_CHUNK = 2048;                      // cloud candidates per workgroup of the count / write passes
constexpr int SP_TW = SVO_SPECKLE_TILE_W, SP_TH = SVO_SPECKLE_TILE_H, SP_PIX = SP_TW * SP_TH, SP_T = 256;  // speckle tile, workgroup
constexpr int SGM_SP = DT_PIX + 2;     // u16 pitch of one SAD plane in LDS: 257 dwords, so the planes of one pixel fall on 64 different banks
constexpr int SGM_T = 256;             // every SGM kernel's workgroup
// dynamic LDS of the SAD planes [ndisp + 1][pitch] of the dense kernels and of sgm_volume_kernel, and the most either asks for
inline size_t dense_sad_lds(int ndisp) { return sizeof(unsigned short) * (size_t)(ndisp + 1) * DT_PIX; }
inline size_t sgm_sad_lds(int ndisp) { return sizeof(unsigned short) * (size_t)(ndisp + 1) * SGM_SP; }
constexpr int DENSE_LDS_MAX = (int)sizeof(unsigned short) * (MAX_NDISP + 1) * DT_PIX;  // 66,560 B
constexpr int SGM_LDS_MAX = (int)sizeof(unsigned short) * (MAX_NDISP + 1) * SGM_SP;    // 66,820 B

// ----------------------------------------------------------------------------- StereoBM: the shape of every entry, the batch of the dense ones
inline int stereo_shape_check(const void* l, const void* r, int W, int H, int stride, int ndisp, int block, int max_width, int max_height,
                              const char** err) {
  DENSE_REFUSE(l && r, "stereo: null image");
  DENSE_REFUSE(W >= 3 && H >= 3 && W <= max_width && H <= max_height && stride >= W, "stereo: image size outside limits");
  DENSE_REFUSE(ndisp >= 16 && ndisp <= MAX_NDISP && ndisp % 16 == 0, "stereo: numDisparities must be 16..64, multiple of 16");
  DENSE_REFUSE(block >= 5 && block <= MAX_BLOCK && (block & 1), "stereo: blockSize must be odd, 5..21");
  return SVO_OK;
}

// null_cost == nullptr: the entry takes no cost map, or takes an optional one
struct DenseBatchTexts { const char *null_disp, *null_cost, *batch, *overlap; };
constexpr DenseBatchTexts STEREO_BM_BATCH_TEXTS = {"stereo_bm_batch: null output", nullptr, "stereo_bm_batch: batch outside 1..max_batch",
                                                   "stereo_bm_batch: images overlap"};
constexpr DenseBatchTexts STEREO_BM_COST_BATCH_TEXTS = {"stereo_bm_cost_batch: null disp16", "stereo_bm_cost_batch: null cost16",
                                                        "stereo_bm_cost_batch: batch outside 1..max_batch", "stereo_bm_cost_batch: images overlap"};
constexpr DenseBatchTexts STEREO_SGM_BATCH_TEXTS = {"stereo_sgm: null disp16", nullptr, "stereo_sgm: batch outside 1..max_batch",
                                                    "stereo_sgm: images overlap (image_stride)"};

// One pair has no neighbour to overlap: image_stride is not looked at.
inline int dense_batch_check(int batch, int max_batch, int W, int H, int row_stride, size_t image_stride, const DenseBatchTexts& t,
                             const char** err) {
  DENSE_REFUSE(batch >= 1 && batch <= max_batch, t.batch);
  DENSE_REFUSE(batch == 1 || image_stride >= (size_t)row_stride * (size_t)(H - 1) + (size_t)W, t.overlap);
  return SVO_OK;
}

// ----------------------------------------------------------------------------- clouds
inline bool cloud_pixels_ok(int W, int H) { return W >= 1 && H >= 1 && (long)W * (long)H <= (1L << 24); }  // the tag's 24 bits

inline int cloud_check(int W, int H, int stride, const svo_camera_info* cam, const svo_cloud_params* prm, int max_width, int max_height,
                       const char** err) {
  DENSE_REFUSE(cam && prm, "cloud: null camera or parameters");
  DENSE_REFUSE(cloud_pixels_ok(W, H), "cloud: width*height must be at most 2^24 (the tag holds the pixel index in 24 bits)");
  DENSE_REFUSE(W <= max_width && H <= max_height && stride >= W, "cloud: image size outside limits");
  DENSE_REFUSE(prm->step >= 1, "cloud: step must be at least 1");
  DENSE_REFUSE(prm->max_points >= 1, "cloud: max_points must be at least 1");
  DENSE_REFUSE(cam->focal != 0.0 && cam->baseline != 0.0, "cloud: focal length and baseline must not be 0");
  return SVO_OK;
}

inline int cloud_default_params(svo_cloud_params* p, int W, int H) {
  if (!p || !cloud_pixels_ok(W, H)) return SVO_ERR_INVALID;
  p->step = 1;
  p->min_disparity = 0.f;
  p->max_points = W * H;
  return SVO_OK;
}

// Candidates: the pixels with x % step == 0 and y % step == 0, in raster order; a chunk is CL_CHUNK of them.
inline int cloud_nx(int W, int step) { return dense_div_up(W, step); }
inline int cloud_n_cand(int W, int H, int step) { return cloud_nx(W, step) * dense_div_up(H, step); }
inline int cloud_chunks(int W, int H, int step) {  // ints of `seg` per image
  const long n = (long)dense_div_up(W, step) * dense_div_up(H, step);
  return (int)((n + CL_CHUNK - 1) / CL_CHUNK);
}
inline size_t cloud_store_cap(int max_points, size_t px) { return (size_t)max_points < px ? (size_t)max_points : px; }  // no more than px points exist

// ----------------------------------------------------------------------------- speckle filter
inline int speckle_shape_check(int W, int H, int batch, const char** err) {
  DENSE_REFUSE(W >= 1 && H >= 1, "speckle_filter: width and height must be at least 1");
  DENSE_REFUSE((long)W * (long)H < (1L << 31), "speckle_filter: width*height must be below 2^31");
  DENSE_REFUSE(batch >= 1 && batch <= 65535, "speckle_filter: batch outside 1..65535");
  return SVO_OK;
}

inline int speckle_check(int W, int H, int batch, const svo_speckle_params* prm, const char** err) {
  if (const int rc = speckle_shape_check(W, H, batch, err)) return rc;
  DENSE_REFUSE(prm, "speckle_filter: null params");
  DENSE_REFUSE(prm->max_size >= 0, "speckle_filter: max_size must not be negative");
  DENSE_REFUSE(prm->max_diff16 >= 0, "speckle_filter: max_diff16 must not be negative");
  return SVO_OK;
}

inline size_t speckle_workspace_bytes(int W, int H, int batch) {  // labels, then counts; 0 for a shape the check refuses
  const char* err = nullptr;
  if (speckle_shape_check(W, H, batch, &err)) return 0;
  return 2 * sizeof(unsigned) * (size_t)W * (size_t)H * (size_t)batch;
}

// Tiles of SP_TW x SP_TH; the seam pairs of an image: first those across the vertical seams, then those across the horizontal ones.
struct SpeckleGrid {
  int tiles_x, tiles_y;
  unsigned n_vert, n_seam;  // seam pairs across vertical seams; all seam pairs (< A / 64 + A / 16)
  unsigned px_blocks;       // workgroups of SP_T over the pixels
};
inline SpeckleGrid speckle_grid(int W, int H) {
  SpeckleGrid g;
  g.tiles_x = dense_div_up(W, SP_TW);
  g.tiles_y = dense_div_up(H, SP_TH);
  g.n_vert = (unsigned)(g.tiles_x - 1) * (unsigned)H;
  g.n_seam = g.n_vert + (unsigned)(g.tiles_y - 1) * (unsigned)W;
  g.px_blocks = (unsigned)(((size_t)W * (size_t)H + SP_T - 1) / SP_T);
  return g;
}

// ----------------------------------------------------------------------------- left-right check
constexpr size_t lr_check_lds(int W) { return 6 * (size_t)W; }  // 4 for the key, 2 for the value
static_assert(lr_check_lds(SVO_LR_CHECK_MAX_WIDTH) <= 64 * 1024 - 64, "key and row must fit the LDS granted without a request");

inline int lr_check_check(int W, int H, int batch, const svo_lr_check_params* prm, const char** err) {
  DENSE_REFUSE(W >= 1, "lr_check: width must be at least 1");
  DENSE_REFUSE(H >= 1, "lr_check: height must be at least 1");
  DENSE_REFUSE(W <= SVO_LR_CHECK_MAX_WIDTH, "lr_check: width exceeds SVO_LR_CHECK_MAX_WIDTH (the row and its keys live in LDS)");
  DENSE_REFUSE(batch >= 1 && batch <= 65535, "lr_check: batch outside 1..65535");
  DENSE_REFUSE(prm, "lr_check: null params");
  DENSE_REFUSE(prm->max_diff16 >= 0, "lr_check: max_diff16 must not be negative");
  return SVO_OK;
}

// ----------------------------------------------------------------------------- semi-global matching
inline int sgm_params_check(const svo_sgm_params* prm, const char** err) {
  DENSE_REFUSE(prm, "stereo_sgm: null params");
  DENSE_REFUSE(prm->p1 >= 0, "stereo_sgm: p1 must not be negative");
  DENSE_REFUSE(prm->p2 >= prm->p1, "stereo_sgm: p2 must be at least p1");
  DENSE_REFUSE(prm->p2 <= SVO_SGM_MAX_P2, "stereo_sgm: p2 exceeds SVO_SGM_MAX_P2 (a path cost must fit 16 bits)");
  return SVO_OK;
}

inline int sgm_default_params(svo_sgm_params* p, int block) {
  if (!p || block < 5 || block > MAX_BLOCK || !(block & 1)) return SVO_ERR_INVALID;
  p->p1 = 2 * block * block;
  p->p2 = 8 * block * block;
  return SVO_OK;
}

// The valid rectangle (where the whole window and every disparity lie inside the image): origin and size; empty when VW or VH <= 0.
struct SgmRect { int rx0, ry0, VW, VH; };
inline SgmRect sgm_rect(int W, int H, int ndisp, int block) { return {ndisp - 1 + block / 2, block / 2, W - block - ndisp + 2, H - block + 1}; }

// The workspace: vol (u16, batch x VH x VW x ndisp), sum (u32, the same count), tex (u16, batch x VH x VW), each 256-byte aligned.
struct SgmLayout { size_t vol, sum, tex, total; };
inline size_t sgm_up(size_t v) { return (v + 255) & ~(size_t)255; }

// false: a shape svo_stereo_sgm_batch_dev refuses
inline bool sgm_layout(int W, int H, int ndisp, int block, int batch, SgmLayout* l) {
  if (W < 3 || H < 3 || batch < 1 || batch > 65535 || ndisp < 16 || ndisp > MAX_NDISP || ndisp % 16 || block < 5 || block > MAX_BLOCK ||
      !(block & 1) || (long)W * (long)H > (1L << 30))
    return false;
  const long vw = (long)W - block - ndisp + 2, vh = (long)H - block + 1;
  const size_t px = (vw > 0 && vh > 0) ? (size_t)vw * (size_t)vh * (size_t)batch : 0;
  l->vol = 0;
  l->sum = sgm_up(px * ndisp * sizeof(uint16_t));
  l->tex = l->sum + sgm_up(px * ndisp * sizeof(uint32_t));
  l->total = l->tex + sgm_up(px * sizeof(uint16_t));
  if (l->total < 256) l->total = 256;  // an empty rectangle needs nothing, but a workspace is never 0 bytes
  return true;
}

inline size_t sgm_workspace_bytes(int W, int H, int ndisp, int block, int batch) {
  SgmLayout l;
  return sgm_layout(W, H, ndisp, block, batch, &l) ? l.total : 0;
}

inline int sgm_check(int W, int H, int ndisp, int block, int batch, const svo_sgm_params* prm, const char** err) {
  if (const int rc = sgm_params_check(prm, err)) return rc;
  SgmLayout l;
  DENSE_REFUSE(sgm_layout(W, H, ndisp, block, batch, &l), "stereo_sgm: width, height, num_disparities, block_size or batch outside the limits");
  return SVO_OK;
}

// Lanes per scanline of the path kernels (48 disparities use 64 with 16 lanes idle), and the workgroups of direction `dir` over one
// pair: a workgroup is SGM_T / 64 wavefronts of 64 / lps scanlines; directions 0, 1 walk rows, 2, 3 walk columns.
inline int sgm_lps(int ndisp) { return ndisp <= 16 ? 16 : ndisp <= 32 ? 32 : 64; }
inline int sgm_path_groups(int dir, const SgmRect& r, int lps) { return dense_div_up(dir < 2 ? r.VH : r.VW, (SGM_T / 64) * (64 / lps)); }

// svo_stereo_sgm's single allocation: the workspace, then the two tight images, the map and the cost map of one pair of px pixels.
struct SgmOneShot { size_t left, right, disp, cost, total; };
inline SgmOneShot sgm_one_shot(size_t workspace_bytes, size_t px) {
  SvoParts parts;
  (void)parts.add(workspace_bytes);  // the workspace comes first, at 0
  SgmOneShot o;
  o.left = parts.add(px);
  o.right = parts.add(px);
  o.disp = parts.add(2 * px);
  o.cost = parts.add(2 * px);
  o.total = parts.total();
  return o;
}

// ----------------------------------------------------------------------------- keyframe clouds of a pipeline / a group
inline int kfc_max_points(int max_points, int W, int H) { return max_points <= 0 ? W * H : max_points; }
inline int kfc_max_keyframes(int max_keyframes, int max_batch) { return max_keyframes == 0 ? max_batch : max_keyframes; }

// *prm: the parameters in force (max_points > 0); *max_kf: the bound in force
inline int kfc_resolve(const svo_cloud_params* params, int W, int H, int max_keyframes, int max_batch, svo_cloud_params* prm, int* max_kf,
                       const char** err) {
  *prm = *params;
  DENSE_REFUSE((long)W * (long)H <= (1L << 24), "set_keyframe_clouds: width*height must be at most 2^24");
  prm->max_points = kfc_max_points(prm->max_points, W, H);
  DENSE_REFUSE(prm->step >= 1, "set_keyframe_clouds: step must be at least 1");
  *max_kf = kfc_max_keyframes(max_keyframes, max_batch);
  DENSE_REFUSE(*max_kf >= 1 && *max_kf <= 65535, "set_keyframe_clouds: max_keyframes_per_call must be 0 or 1..65535");
  return SVO_OK;
}

// Every buffer of svo_kfc_create for max_kf keyframes (pinned: [max_kf pairs | max_kf x 2 counts]), and the cost maps of the
// left-right switch.  The speckle switch allocates speckle_workspace_bytes(W, H, max_kf); the SGM switch sgm_workspace_bytes for
// SVO_SGM_KEYFRAME_SUB_BATCH pairs, whatever max_kf is.
constexpr size_t KFC_PAIR_BYTES = 2 * sizeof(void*);  // one (left, right) record of the pair table
struct KfcBytes { size_t disp, points, counts, seg, tab, pinned; };
inline KfcBytes kfc_bytes(int W, int H, const svo_cloud_params& prm, int max_kf) {
  const size_t px = (size_t)W * (size_t)H, n = (size_t)max_kf;
  KfcBytes b;
  b.disp = n * px * sizeof(int16_t);
  b.points = n * (size_t)prm.max_points * sizeof(svo_cloud_point);
  b.counts = n * 2 * sizeof(int);
  b.seg = n * (size_t)cloud_chunks(W, H, prm.step) * sizeof(int);
  b.tab = n * KFC_PAIR_BYTES;
  b.pinned = n * (KFC_PAIR_BYTES + 2 * sizeof(int));
  return b;
}
inline size_t kfc_cost_bytes(int W, int H, int max_kf) { return sizeof(uint16_t) * (size_t)W * (size_t)H * (size_t)max_kf; }

// The SGM sequence runs per sub-batch: the pairs b0 .. b0 + kfc_sub_batch(n, b0) - 1 for b0 = 0, SUB, 2 SUB, ... < n.
inline int kfc_sub_batch(int n, int b0) { return n - b0 < SVO_SGM_KEYFRAME_SUB_BATCH ? n - b0 : SVO_SGM_KEYFRAME_SUB_BATCH; }

#endif  // SVO_DENSE_ARGS_H_
