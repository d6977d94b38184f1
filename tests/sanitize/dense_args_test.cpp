// The dense keyframe chain's GPU-free host logic (stereo_vo_amd/host/dense_args.h) walked on the host, under ASan + UBSan: every
// rule accepted at its limit and refused one step beyond with its code and its exact message, the chunk and seam counts against
// brute-force counts, the SGM workspace's regions, the path grid, and the sizes and the sub-batch split of the keyframe clouds.
#include <limits.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "dense_args.h"

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { ++fails; fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

// rc is the refusal with exactly this message, or (want == nullptr) SVO_OK with the message untouched
static void expect(int rc, const char* err, const char* want, const char* where) {
  if (want) CHECK(rc == SVO_ERR_INVALID && err && strcmp(err, want) == 0, "%s: rc %d, message '%s', wanted '%s'", where, rc, err ? err : "(none)", want);
  else CHECK(rc == SVO_OK && err == nullptr, "%s: rc %d, message '%s', wanted acceptance", where, rc, err ? err : "(none)");
}

// the check runs first: its message is read only after it returned
#define EXPECT(call, want, where) do { const char* err = nullptr; const int rc_ = (call); expect(rc_, err, want, where); } while (0)

static const unsigned char IMG[1] = {0};
constexpr int MAXW = 2048, MAXH = 1024, MAXB = 8;  // a context's limits

static void stereo_shape() {
  const char* null_image = "stereo: null image";
  const char* size = "stereo: image size outside limits";
  const char* nd = "stereo: numDisparities must be 16..64, multiple of 16";
  const char* bs = "stereo: blockSize must be odd, 5..21";
  auto shape = [&](int W, int H, int stride, int ndisp, int block, const char** err) {
    return stereo_shape_check(IMG, IMG, W, H, stride, ndisp, block, MAXW, MAXH, err);
  };
  EXPECT(stereo_shape_check(nullptr, IMG, 64, 64, 64, 16, 5, MAXW, MAXH, &err), null_image, "null left");
  EXPECT(stereo_shape_check(IMG, nullptr, 64, 64, 64, 16, 5, MAXW, MAXH, &err), null_image, "null right");
  EXPECT(stereo_shape_check(nullptr, IMG, 2, 64, 64, 0, 4, MAXW, MAXH, &err), null_image, "the null image comes first");
  EXPECT(shape(2, 64, 64, 16, 5, &err), size, "W = 2");
  EXPECT(shape(3, 64, 64, 16, 5, &err), nullptr, "W = 3");
  EXPECT(shape(64, 2, 64, 16, 5, &err), size, "H = 2");
  EXPECT(shape(64, 3, 64, 16, 5, &err), nullptr, "H = 3");
  EXPECT(shape(MAXW, MAXH, MAXW, 16, 5, &err), nullptr, "the limits");
  EXPECT(shape(MAXW + 1, 64, MAXW + 1, 16, 5, &err), size, "max_width + 1");
  EXPECT(shape(64, MAXH + 1, 64, 16, 5, &err), size, "max_height + 1");
  EXPECT(shape(64, 64, 63, 16, 5, &err), size, "stride = W - 1");
  EXPECT(shape(64, 64, 64, 16, 5, &err), nullptr, "stride = W");
  EXPECT(shape(2, 64, 64, 0, 4, &err), size, "the size comes before the range and the block");
  for (int n : {0, 8, 24, 80}) EXPECT(shape(64, 64, 64, n, 5, &err), nd, "ndisp refused");
  for (int n : {16, 64}) EXPECT(shape(64, 64, 64, n, 5, &err), nullptr, "ndisp accepted");
  EXPECT(shape(64, 64, 64, 0, 4, &err), nd, "the range comes before the block");
  for (int b : {3, 6, 23}) EXPECT(shape(64, 64, 64, 16, b, &err), bs, "block refused");
  for (int b : {5, 21}) EXPECT(shape(64, 64, 64, 16, b, &err), nullptr, "block accepted");
  CHECK(MAX_NDISP == 64 && MAX_BLOCK == 21, "limits");
  CHECK(dense_sad_lds(MAX_NDISP) == (size_t)DENSE_LDS_MAX && DENSE_LDS_MAX == 66560, "dense LDS %d", DENSE_LDS_MAX);
  CHECK(sgm_sad_lds(MAX_NDISP) == (size_t)SGM_LDS_MAX && SGM_LDS_MAX == 66820, "sgm LDS %d", SGM_LDS_MAX);
  CHECK(dense_sad_lds(16) == 2u * 17 * 512 && sgm_sad_lds(16) == 2u * 17 * 514, "LDS at 16 disparities");
}

static void batch_rule() {
  const struct { const DenseBatchTexts* t; const char *null_disp, *null_cost, *batch, *overlap; } entries[] = {
      {&STEREO_BM_BATCH_TEXTS, "stereo_bm_batch: null output", nullptr, "stereo_bm_batch: batch outside 1..max_batch", "stereo_bm_batch: images overlap"},
      {&STEREO_BM_COST_BATCH_TEXTS, "stereo_bm_cost_batch: null disp16", "stereo_bm_cost_batch: null cost16",
       "stereo_bm_cost_batch: batch outside 1..max_batch", "stereo_bm_cost_batch: images overlap"},
      {&STEREO_SGM_BATCH_TEXTS, "stereo_sgm: null disp16", nullptr, "stereo_sgm: batch outside 1..max_batch", "stereo_sgm: images overlap (image_stride)"}};
  const int W = 70, H = 25, stride = 96;
  const size_t tight = (size_t)stride * (H - 1) + W;
  for (const auto& e : entries) {
    CHECK(strcmp(e.t->null_disp, e.null_disp) == 0, "null_disp text '%s'", e.t->null_disp);
    CHECK(e.null_cost ? e.t->null_cost && strcmp(e.t->null_cost, e.null_cost) == 0 : e.t->null_cost == nullptr, "null_cost text of %s", e.null_disp);
    EXPECT(dense_batch_check(0, MAXB, W, H, stride, tight, *e.t, &err), e.batch, "batch 0");
    EXPECT(dense_batch_check(1, MAXB, W, H, stride, tight, *e.t, &err), nullptr, "batch 1");
    EXPECT(dense_batch_check(MAXB, MAXB, W, H, stride, tight, *e.t, &err), nullptr, "max_batch");
    EXPECT(dense_batch_check(MAXB + 1, MAXB, W, H, stride, tight, *e.t, &err), e.batch, "max_batch + 1");
    EXPECT(dense_batch_check(2, MAXB, W, H, stride, tight, *e.t, &err), nullptr, "batch 2, images touch");
    EXPECT(dense_batch_check(2, MAXB, W, H, stride, tight - 1, *e.t, &err), e.overlap, "batch 2, one byte shared");
    EXPECT(dense_batch_check(1, MAXB, W, H, stride, tight - 1, *e.t, &err), nullptr, "batch 1 does not look at image_stride");
    EXPECT(dense_batch_check(1, MAXB, W, H, stride, 0, *e.t, &err), nullptr, "batch 1, image_stride 0");
    EXPECT(dense_batch_check(0, MAXB, W, H, stride, 0, *e.t, &err), e.batch, "the batch comes before the overlap");
  }
}

static void cloud() {
  const char* px = "cloud: width*height must be at most 2^24 (the tag holds the pixel index in 24 bits)";
  const svo_camera_info cam = {700.0, 600.0, 180.0, 0, 0, 0, 0, 0.5};
  const svo_cloud_params ok = {1, 0.f, 1};
  auto check = [&](int W, int H, int stride, const svo_camera_info* c, const svo_cloud_params* p, const char** err) {
    return cloud_check(W, H, stride, c, p, 8192, 8192, err);
  };
  EXPECT(check(64, 64, 64, nullptr, &ok, &err), "cloud: null camera or parameters", "null camera");
  EXPECT(check(64, 64, 64, &cam, nullptr, &err), "cloud: null camera or parameters", "null parameters");
  EXPECT(check(4096, 4096, 4096, &cam, &ok, &err), nullptr, "2^24 pixels");
  EXPECT(check(4097, 4096, 4097, &cam, &ok, &err), px, "2^24 + 4096 pixels");
  EXPECT(check(0, 64, 64, &cam, &ok, &err), px, "W = 0");
  EXPECT(check(64, 0, 64, &cam, &ok, &err), px, "H = 0");
  EXPECT(check(1, 1, 1, &cam, &ok, &err), nullptr, "one pixel");
  EXPECT(check(8193, 1, 8193, &cam, &ok, &err), "cloud: image size outside limits", "max_width + 1");
  EXPECT(check(1, 8193, 1, &cam, &ok, &err), "cloud: image size outside limits", "max_height + 1");
  EXPECT(check(64, 64, 63, &cam, &ok, &err), "cloud: image size outside limits", "stride = W - 1");
  svo_cloud_params p = ok;
  p.step = 0;
  EXPECT(check(64, 64, 64, &cam, &p, &err), "cloud: step must be at least 1", "step 0");
  p.max_points = 0;
  EXPECT(check(64, 64, 64, &cam, &p, &err), "cloud: step must be at least 1", "the step comes before max_points");
  p.step = 1;
  EXPECT(check(64, 64, 64, &cam, &p, &err), "cloud: max_points must be at least 1", "max_points 0");
  svo_camera_info c = cam;
  c.focal = 0.0;
  EXPECT(check(64, 64, 64, &c, &ok, &err), "cloud: focal length and baseline must not be 0", "focal 0");
  c = cam;
  c.baseline = 0.0;
  EXPECT(check(64, 64, 64, &c, &ok, &err), "cloud: focal length and baseline must not be 0", "baseline 0");
  c.baseline = -0.5;
  EXPECT(check(64, 64, 64, &c, &ok, &err), nullptr, "a negative baseline is not 0");

  svo_cloud_params d = {7, 7.f, 7};
  CHECK(cloud_default_params(&d, 4096, 4096) == SVO_OK && d.step == 1 && d.min_disparity == 0.f && d.max_points == 1 << 24, "defaults at 2^24");
  d = {7, 7.f, 7};
  CHECK(cloud_default_params(&d, 4097, 4096) == SVO_ERR_INVALID && d.step == 7 && d.max_points == 7, "defaults beyond 2^24");
  CHECK(cloud_default_params(&d, 0, 64) == SVO_ERR_INVALID && cloud_default_params(&d, 64, 0) == SVO_ERR_INVALID, "defaults of an empty image");
  CHECK(cloud_default_params(nullptr, 64, 64) == SVO_ERR_INVALID, "defaults into null");

  const int shapes[][3] = {{1, 1, 1}, {64, 8, 1}, {65, 9, 2}, {496, 160, 3}, {4096, 4096, 1}};
  for (const auto& s : shapes) {
    const int W = s[0], H = s[1], step = s[2];
    long nx = 0, n = 0;
    for (int x = 0; x < W; ++x) nx += x % step == 0;
    for (int y = 0; y < H; ++y)
      if (y % step == 0) n += nx;
    long chunks = 0;
    for (long k = 0; k < n; k += CL_CHUNK) ++chunks;
    CHECK(cloud_nx(W, step) == nx && cloud_n_cand(W, H, step) == n && cloud_chunks(W, H, step) == chunks,
          "%d x %d step %d: nx %d (%ld), n_cand %d (%ld), chunks %d (%ld)", W, H, step, cloud_nx(W, step), nx, cloud_n_cand(W, H, step), n,
          cloud_chunks(W, H, step), chunks);
  }
  CHECK(CL_CHUNK == 2048 && cloud_chunks(4096, 4096, 1) == 8192, "chunk size");
  CHECK(cloud_store_cap(5, 100) == 5 && cloud_store_cap(100, 100) == 100 && cloud_store_cap(101, 100) == 100 && cloud_store_cap(INT_MAX, 9) == 9, "store cap");
}

static void speckle() {
  const char* shape = "speckle_filter: width and height must be at least 1";
  const char* px = "speckle_filter: width*height must be below 2^31";
  const char* batch = "speckle_filter: batch outside 1..65535";
  const svo_speckle_params ok = {100, 16};
  EXPECT(speckle_check(0, 5, 1, &ok, &err), shape, "W = 0");
  EXPECT(speckle_check(5, 0, 1, &ok, &err), shape, "H = 0");
  EXPECT(speckle_check(1, 1, 1, &ok, &err), nullptr, "one pixel");
  EXPECT(speckle_check(65536, 32767, 1, &ok, &err), nullptr, "2^31 - 65536 pixels");
  EXPECT(speckle_check(65536, 32768, 1, &ok, &err), px, "2^31 pixels");
  EXPECT(speckle_check(64, 64, 0, &ok, &err), batch, "batch 0");
  EXPECT(speckle_check(64, 64, 65535, &ok, &err), nullptr, "batch 65535");
  EXPECT(speckle_check(64, 64, 65536, &ok, &err), batch, "batch 65536");
  EXPECT(speckle_check(65536, 32768, 0, &ok, &err), px, "the pixels come before the batch");
  EXPECT(speckle_check(64, 64, 1, nullptr, &err), "speckle_filter: null params", "null params");
  EXPECT(speckle_check(64, 64, 0, nullptr, &err), batch, "the batch comes before the params");
  svo_speckle_params p = {-1, -1};
  EXPECT(speckle_check(64, 64, 1, &p, &err), "speckle_filter: max_size must not be negative", "max_size -1 (before max_diff16)");
  p = {0, -1};
  EXPECT(speckle_check(64, 64, 1, &p, &err), "speckle_filter: max_diff16 must not be negative", "max_diff16 -1");
  p = {0, 0};
  EXPECT(speckle_check(64, 64, 1, &p, &err), nullptr, "both 0");
  p = {INT_MAX, INT_MAX};
  EXPECT(speckle_check(64, 64, 1, &p, &err), nullptr, "both INT_MAX");

  CHECK(speckle_workspace_bytes(64, 64, 1) == 8u * 64 * 64, "bytes of one tile row");
  CHECK(speckle_workspace_bytes(131, 37, 3) == 8u * 131 * 37 * 3, "bytes of an odd shape");
  CHECK(speckle_workspace_bytes(65536, 32767, 65535) == (size_t)8 * 65536 * 32767 * 65535, "bytes at the largest shape and batch");
  CHECK(speckle_workspace_bytes(65536, 32768, 1) == 0 && speckle_workspace_bytes(0, 1, 1) == 0 && speckle_workspace_bytes(1, 0, 1) == 0 &&
            speckle_workspace_bytes(64, 64, 0) == 0 && speckle_workspace_bytes(64, 64, 65536) == 0, "bytes of a refused shape");

  CHECK(SP_TW == 64 && SP_TH == 16 && SP_PIX == 1024 && SP_T == 256, "tile figures");
  for (int W : {1, SP_TW, SP_TW + 1, 131})
    for (int H : {1, SP_TH, SP_TH + 1, 37}) {
      // brute force: the 4-neighbour pairs whose two pixels lie in different tiles
      unsigned vert = 0, horz = 0;
      int tx = 0, ty = 0;
      for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
          if (x > 0 && (x - 1) / SP_TW != x / SP_TW) ++vert;
          if (y > 0 && (y - 1) / SP_TH != y / SP_TH) ++horz;
          tx = std::max(tx, x / SP_TW + 1);
          ty = std::max(ty, y / SP_TH + 1);
        }
      const SpeckleGrid g = speckle_grid(W, H);
      unsigned blocks = 0;
      for (long p = 0; p < (long)W * H; p += SP_T) ++blocks;
      CHECK(g.tiles_x == tx && g.tiles_y == ty && g.n_vert == vert && g.n_seam == vert + horz && g.px_blocks == blocks,
            "%d x %d: tiles %d x %d (%d x %d), n_vert %u (%u), n_seam %u (%u), px_blocks %u (%u)", W, H, g.tiles_x, g.tiles_y, tx, ty, g.n_vert, vert,
            g.n_seam, vert + horz, g.px_blocks, blocks);
    }
  const SpeckleGrid big = speckle_grid(65536, 32767);  // the largest shape: every figure in range (UBSan sees the arithmetic)
  CHECK(big.tiles_x == 1024 && big.tiles_y == 2048 && big.n_vert == 1023u * 32767u && big.n_seam == 1023u * 32767u + 2047u * 65536u &&
            big.px_blocks == 8388352u, "grid of the largest shape");
}

static void lr_check() {
  const char* batch = "lr_check: batch outside 1..65535";
  const svo_lr_check_params ok = {16};
  EXPECT(lr_check_check(0, 5, 1, &ok, &err), "lr_check: width must be at least 1", "W = 0");
  EXPECT(lr_check_check(0, 0, 1, &ok, &err), "lr_check: width must be at least 1", "the width comes before the height");
  EXPECT(lr_check_check(5, 0, 1, &ok, &err), "lr_check: height must be at least 1", "H = 0");
  EXPECT(lr_check_check(1, 1, 1, &ok, &err), nullptr, "one pixel");
  EXPECT(lr_check_check(SVO_LR_CHECK_MAX_WIDTH, 4, 1, &ok, &err), nullptr, "the widest row");
  EXPECT(lr_check_check(SVO_LR_CHECK_MAX_WIDTH + 1, 4, 1, &ok, &err), "lr_check: width exceeds SVO_LR_CHECK_MAX_WIDTH (the row and its keys live in LDS)",
         "one column more");
  EXPECT(lr_check_check(64, 64, 0, &ok, &err), batch, "batch 0");
  EXPECT(lr_check_check(64, 64, 65535, &ok, &err), nullptr, "batch 65535");
  EXPECT(lr_check_check(64, 64, 65536, &ok, &err), batch, "batch 65536");
  EXPECT(lr_check_check(64, 64, 1, nullptr, &err), "lr_check: null params", "null params");
  EXPECT(lr_check_check(64, 64, 0, nullptr, &err), batch, "the batch comes before the params");
  svo_lr_check_params p = {-1};
  EXPECT(lr_check_check(64, 64, 1, &p, &err), "lr_check: max_diff16 must not be negative", "max_diff16 -1");
  p = {0};
  EXPECT(lr_check_check(64, 64, 1, &p, &err), nullptr, "max_diff16 0");
  CHECK(lr_check_lds(1) == 6 && lr_check_lds(SVO_LR_CHECK_MAX_WIDTH) == 6u * SVO_LR_CHECK_MAX_WIDTH && lr_check_lds(SVO_LR_CHECK_MAX_WIDTH) <= 64 * 1024 - 64,
        "LDS of the widest row: %zu", lr_check_lds(SVO_LR_CHECK_MAX_WIDTH));
}

static void sgm_params() {
  svo_sgm_params p = {-1, 5};
  EXPECT(sgm_params_check(nullptr, &err), "stereo_sgm: null params", "null params");
  EXPECT(sgm_params_check(&p, &err), "stereo_sgm: p1 must not be negative", "p1 -1");
  p = {0, 0};
  EXPECT(sgm_params_check(&p, &err), nullptr, "both 0");
  p = {10, 9};
  EXPECT(sgm_params_check(&p, &err), "stereo_sgm: p2 must be at least p1", "p2 = p1 - 1");
  p = {10, 10};
  EXPECT(sgm_params_check(&p, &err), nullptr, "p2 = p1");
  p = {SVO_SGM_MAX_P2, SVO_SGM_MAX_P2};
  EXPECT(sgm_params_check(&p, &err), nullptr, "both SVO_SGM_MAX_P2");
  p = {10, SVO_SGM_MAX_P2 + 1};
  EXPECT(sgm_params_check(&p, &err), "stereo_sgm: p2 exceeds SVO_SGM_MAX_P2 (a path cost must fit 16 bits)", "SVO_SGM_MAX_P2 + 1");
  p = {SVO_SGM_MAX_P2 + 2, SVO_SGM_MAX_P2 + 1};
  EXPECT(sgm_params_check(&p, &err), "stereo_sgm: p2 must be at least p1", "p2 < p1 comes before the bound");
  for (int b : {4, 22, 23}) {
    svo_sgm_params d = {-7, -7};
    CHECK(sgm_default_params(&d, b) == SVO_ERR_INVALID && d.p1 == -7 && d.p2 == -7, "defaults for block %d", b);
  }
  for (int b : {5, 21}) {
    svo_sgm_params d = {-7, -7};
    CHECK(sgm_default_params(&d, b) == SVO_OK && d.p1 == 2 * b * b && d.p2 == 8 * b * b, "defaults for block %d: %d, %d", b, d.p1, d.p2);
    EXPECT(sgm_params_check(&d, &err), nullptr, "the defaults pass the check");
  }
  CHECK(sgm_default_params(nullptr, 21) == SVO_ERR_INVALID, "defaults into null");
  // the whole check: the parameters first, then the shape
  const char* shape = "stereo_sgm: width, height, num_disparities, block_size or batch outside the limits";
  const svo_sgm_params ok = {8, 32};
  p = {-1, 0};
  EXPECT(sgm_check(2, 2, 16, 5, 1, &p, &err), "stereo_sgm: p1 must not be negative", "the parameters come before the shape");
  EXPECT(sgm_check(2, 64, 16, 5, 1, &ok, &err), shape, "W = 2");
  EXPECT(sgm_check(3, 3, 16, 5, 1, &ok, &err), nullptr, "3 x 3");
}

static void sgm_layout_rules() {
  SgmLayout l;
  const struct { int W, H, ndisp, block, batch; bool ok; const char* what; } cases[] = {
      {2, 64, 16, 5, 1, false, "W = 2"}, {3, 64, 16, 5, 1, true, "W = 3"}, {64, 2, 16, 5, 1, false, "H = 2"}, {64, 3, 16, 5, 1, true, "H = 3"},
      {64, 64, 16, 5, 0, false, "batch 0"}, {64, 64, 16, 5, 1, true, "batch 1"}, {64, 64, 16, 5, 65535, true, "batch 65535"},
      {64, 64, 16, 5, 65536, false, "batch 65536"}, {64, 64, 0, 5, 1, false, "ndisp 0"}, {64, 64, 15, 5, 1, false, "ndisp 15"},
      {64, 64, 16, 5, 1, true, "ndisp 16"}, {64, 64, 17, 5, 1, false, "ndisp 17"}, {64, 64, 24, 5, 1, false, "ndisp 24"},
      {64, 64, 64, 5, 1, true, "ndisp 64"}, {64, 64, 80, 5, 1, false, "ndisp 80"}, {64, 64, 16, 3, 1, false, "block 3"},
      {64, 64, 16, 4, 1, false, "block 4"}, {64, 64, 16, 5, 1, true, "block 5"}, {64, 64, 16, 6, 1, false, "block 6"},
      {64, 64, 16, 21, 1, true, "block 21"}, {64, 64, 16, 22, 1, false, "block 22"}, {64, 64, 16, 23, 1, false, "block 23"},
      {32768, 32768, 64, 21, 1, true, "2^30 pixels"}, {32769, 32768, 64, 21, 1, false, "2^30 + 32768 pixels"},
      {65536, 16384, 16, 5, 1, true, "2^30 pixels, wide"}, {65536, 16385, 16, 5, 1, false, "2^30 + 65536 pixels"}};
  for (const auto& c : cases) {
    const bool ok = sgm_layout(c.W, c.H, c.ndisp, c.block, c.batch, &l);
    CHECK(ok == c.ok, "sgm_layout %s: %d", c.what, (int)ok);
    CHECK((sgm_workspace_bytes(c.W, c.H, c.ndisp, c.block, c.batch) != 0) == c.ok, "sgm_workspace_bytes %s", c.what);
  }
  CHECK(sgm_up(0) == 0 && sgm_up(1) == 256 && sgm_up(256) == 256 && sgm_up(257) == 512, "sgm_up");

  const int shapes[][5] = {{70, 25, 16, 5, 3}, {496, 160, 48, 21, 2}, {32768, 32768, 64, 21, 1}};
  for (const auto& s : shapes) {
    const int W = s[0], H = s[1], ndisp = s[2], block = s[3], batch = s[4];
    CHECK(sgm_layout(W, H, ndisp, block, batch, &l), "layout of %d x %d", W, H);
    const SgmRect r = sgm_rect(W, H, ndisp, block);
    // the rectangle: x in [rx0, rx0 + VW) are the columns whose window and whose whole disparity range lie inside the image
    int vw = 0, vh = 0, x0 = -1, y0 = -1;
    for (int x = 0; x < W; ++x)
      if (x - block / 2 - (ndisp - 1) >= 0 && x + block / 2 < W) { if (x0 < 0) x0 = x; ++vw; }
    for (int y = 0; y < H; ++y)
      if (y - block / 2 >= 0 && y + block / 2 < H) { if (y0 < 0) y0 = y; ++vh; }
    CHECK(r.rx0 == x0 && r.ry0 == y0 && r.VW == vw && r.VH == vh, "%d x %d: rectangle (%d, %d) %d x %d, wanted (%d, %d) %d x %d", W, H, r.rx0, r.ry0,
          r.VW, r.VH, x0, y0, vw, vh);
    const size_t px = (size_t)vw * (size_t)vh * (size_t)batch;
    const size_t need[3] = {px * ndisp * 2, px * ndisp * 4, px * 2}, at[4] = {l.vol, l.sum, l.tex, l.total};
    for (int i = 0; i < 3; ++i)
      CHECK(at[i] % 256 == 0 && at[i] + need[i] <= at[i + 1], "%d x %d: region %d at %zu needs %zu, the next begins at %zu", W, H, i, at[i], need[i], at[i + 1]);
    CHECK(l.vol == 0 && l.total % 256 == 0 && l.total == sgm_workspace_bytes(W, H, ndisp, block, batch), "%d x %d: total %zu", W, H, l.total);
  }
  // an empty rectangle: a workspace is never 0 bytes
  CHECK(sgm_layout(5 + 16 - 2, 25, 16, 5, 3, &l) && l.total == 256 && sgm_rect(5 + 16 - 2, 25, 16, 5).VW == 0, "empty rectangle: %zu", l.total);
  CHECK(sgm_layout(5 + 16 - 1, 25, 16, 5, 1, &l) && l.total == 256 * (size_t)((21 * 32 + 255) / 256 + (21 * 64 + 255) / 256 + 1), "one column: %zu", l.total);
  CHECK(sgm_layout(64, 4, 16, 5, 1, &l) && l.total == 256 && sgm_rect(64, 4, 16, 5).VH == 0, "no row: %zu", l.total);

  const int lps_of[][2] = {{16, 16}, {32, 32}, {48, 64}, {64, 64}};
  for (const auto& p : lps_of) {
    const int ndisp = p[0], lps = sgm_lps(ndisp);
    CHECK(lps == p[1], "lps of %d: %d", ndisp, lps);
    for (const auto& s : shapes) {
      if (s[0] < 21 + ndisp) continue;
      const SgmRect r = sgm_rect(s[0], s[1], ndisp, 21);
      for (int dir = 0; dir < 4; ++dir) {
        const int lines = dir < 2 ? r.VH : r.VW, per = 4 * 64 / lps;
        int groups = 0;
        for (int k = 0; k < lines; k += per) ++groups;
        CHECK(sgm_path_groups(dir, r, lps) == groups, "%d x %d, %d disparities, direction %d: %d groups, wanted %d", s[0], s[1], ndisp, dir,
              sgm_path_groups(dir, r, lps), groups);
      }
    }
  }
  CHECK(SGM_T == 256 && SGM_SP == DT_PIX + 2, "SGM figures");

  // the one-shot entry: workspace, left, right, map, cost map
  for (const auto& s : shapes) {
    const size_t px = (size_t)s[0] * (size_t)s[1], ws = sgm_workspace_bytes(s[0], s[1], s[2], s[3], 1);
    const SgmOneShot o = sgm_one_shot(ws, px);
    const size_t at[6] = {0, o.left, o.right, o.disp, o.cost, o.total}, need[5] = {ws, px, px, 2 * px, 2 * px};
    for (int i = 0; i < 5; ++i)
      CHECK(at[i] % 256 == 0 && at[i] + need[i] <= at[i + 1], "one shot of %d x %d: region %d at %zu needs %zu, the next begins at %zu", s[0], s[1], i, at[i],
            need[i], at[i + 1]);
  }
}

static void keyframe_clouds() {
  const char* kf = "set_keyframe_clouds: max_keyframes_per_call must be 0 or 1..65535";
  svo_cloud_params prm;
  int max_kf = -9;
  const svo_cloud_params in = {2, 0.5f, 0};
  EXPECT(kfc_resolve(&in, 496, 160, 0, MAXB, &prm, &max_kf, &err), nullptr, "max_keyframes 0");
  CHECK(max_kf == MAXB && prm.max_points == 496 * 160 && prm.step == 2 && prm.min_disparity == 0.5f, "resolved: %d keyframes, %d points", max_kf, prm.max_points);
  EXPECT(kfc_resolve(&in, 496, 160, 65535, MAXB, &prm, &max_kf, &err), nullptr, "max_keyframes 65535");
  CHECK(max_kf == 65535, "65535 stays: %d", max_kf);
  EXPECT(kfc_resolve(&in, 496, 160, 1, MAXB, &prm, &max_kf, &err), nullptr, "max_keyframes 1");
  EXPECT(kfc_resolve(&in, 496, 160, 65536, MAXB, &prm, &max_kf, &err), kf, "max_keyframes 65536");
  EXPECT(kfc_resolve(&in, 496, 160, -1, MAXB, &prm, &max_kf, &err), kf, "max_keyframes -1");
  svo_cloud_params p = {1, 0.f, -5};
  EXPECT(kfc_resolve(&p, 496, 160, 3, MAXB, &prm, &max_kf, &err), nullptr, "max_points -5");
  CHECK(prm.max_points == 496 * 160 && max_kf == 3, "max_points -5 -> %d", prm.max_points);
  p.max_points = 496 * 160 - 1;
  EXPECT(kfc_resolve(&p, 496, 160, 3, MAXB, &prm, &max_kf, &err), nullptr, "max_points given");
  CHECK(prm.max_points == 496 * 160 - 1, "max_points given -> %d", prm.max_points);
  CHECK(kfc_max_points(0, 7, 5) == 35 && kfc_max_points(-5, 7, 5) == 35 && kfc_max_points(1, 7, 5) == 1, "kfc_max_points");
  CHECK(kfc_max_keyframes(0, MAXB) == MAXB && kfc_max_keyframes(3, MAXB) == 3 && kfc_max_keyframes(-1, MAXB) == -1, "kfc_max_keyframes");
  p = {0, 0.f, 0};
  EXPECT(kfc_resolve(&p, 496, 160, 0, MAXB, &prm, &max_kf, &err), "set_keyframe_clouds: step must be at least 1", "step 0");
  EXPECT(kfc_resolve(&p, 496, 160, -1, MAXB, &prm, &max_kf, &err), "set_keyframe_clouds: step must be at least 1", "the step comes before the bound");
  EXPECT(kfc_resolve(&in, 4096, 4096, 0, MAXB, &prm, &max_kf, &err), nullptr, "2^24 pixels");
  EXPECT(kfc_resolve(&p, 4097, 4096, 0, MAXB, &prm, &max_kf, &err), "set_keyframe_clouds: width*height must be at most 2^24", "the pixels come first");

  const svo_cloud_params q = {3, 0.f, 1000};
  const KfcBytes b = kfc_bytes(496, 160, q, 5);
  CHECK(b.disp == 5u * 496 * 160 * 2 && b.points == 5u * 1000 * 16 && b.counts == 5u * 2 * 4 && b.seg == 5u * 4 * (size_t)cloud_chunks(496, 160, 3) &&
            b.tab == 5u * 2 * sizeof(void*) && b.pinned == 5u * (2 * sizeof(void*) + 8), "buffers of 5 keyframes");
  static_assert(sizeof(svo_cloud_point) == 16, "a cloud record");
  const svo_cloud_params full = {1, 0.f, 1 << 24};
  const KfcBytes big = kfc_bytes(4096, 4096, full, 65535);  // the largest object: UBSan sees the arithmetic
  CHECK(big.disp == (size_t)65535 * 2 << 24 && big.points == (size_t)65535 * 16 << 24 && big.seg == (size_t)65535 * 4 * 8192, "buffers of the largest object");
  CHECK(kfc_cost_bytes(496, 160, 5) == 5u * 496 * 160 * 2 && kfc_cost_bytes(4096, 4096, 65535) == (size_t)65535 * 2 << 24, "cost maps");

  const int SUB = SVO_SGM_KEYFRAME_SUB_BATCH;
  for (int n : {0, 1, SUB, SUB + 1, 2 * SUB}) {
    std::vector<int> seen;
    int calls = 0;
    for (int b0 = 0; b0 < n; b0 += SUB, ++calls) {
      const int nb = kfc_sub_batch(n, b0);
      CHECK(nb >= 1 && nb <= SUB, "n = %d: a sub-batch of %d at %d", n, nb, b0);
      for (int i = 0; i < nb; ++i) seen.push_back(b0 + i);
    }
    bool in_order = (int)seen.size() == n;
    for (int i = 0; in_order && i < n; ++i) in_order = seen[(size_t)i] == i;
    CHECK(in_order && calls == (n + SUB - 1) / SUB, "n = %d: %zu indices in %d sub-batches", n, seen.size(), calls);
  }
}

int main() {
  stereo_shape();
  batch_rule();
  cloud();
  speckle();
  lr_check();
  sgm_params();
  sgm_layout_rules();
  keyframe_clouds();
  if (fails) { fprintf(stderr, "%d check(s) failed\n", fails); return 1; }
  printf("dense args ok\n");
  return 0;
}
