// The voxel map's GPU-free host logic (stereo_vo_amd/host/voxel_args.h) walked on the host, under ASan + UBSan: every refusal at its
// boundary with its code and its exact message, the accepted side of each boundary, the table's size, the two matrices of a pose7,
// the copy's box -> key range, and the launch geometry.
#include <limits.h>
#include <stdio.h>
#include <string.h>

#include <limits>
#include <random>

#include "voxel_args.h"

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { ++fails; fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

// rc is the refusal with exactly this message, or (want == nullptr) SVO_OK with the message untouched
static void expect(int rc, const char* err, const char* want, const char* where) {
  if (want) CHECK(rc == SVO_ERR_INVALID && err && strcmp(err, want) == 0, "%s: rc %d, message '%s', wanted '%s'", where, rc, err ? err : "(none)", want);
  else CHECK(rc == SVO_OK && err == nullptr, "%s: rc %d, message '%s', wanted acceptance", where, rc, err ? err : "(none)");
}

// the check runs first: its message is read only after it returned
#define EXPECT(call, want, where) do { const char* err = nullptr; const int rc_ = (call); expect(rc_, err, want, where); } while (0)

static const double NaN = std::numeric_limits<double>::quiet_NaN(), Inf = std::numeric_limits<double>::infinity();

static void map_params() {
  const char* size = "voxel_map_create: voxel_size must be finite and > 0";
  const char* cap = "voxel_map_create: capacity_log2 outside 8..28";
  const struct { float vs; int lg; const char* want; } cases[] = {
      {0.0f, 10, size}, {-0.1f, 10, size}, {(float)NaN, 10, size}, {(float)Inf, 10, size}, {FLT_MAX, 10, nullptr}, {FLT_MIN, 10, nullptr},
      {0.1f, 7, cap}, {0.1f, 8, nullptr}, {0.1f, 28, nullptr}, {0.1f, 29, cap}};
  for (const auto& c : cases) {
    const svo_voxel_map_params p = {c.vs, c.lg, 0.0f};
    EXPECT(voxel_params_check(&p, &err), c.want, "map params");
    size_t bytes = 77;
    const int rc = voxel_table_bytes(&p, &bytes);
    CHECK(rc == (c.want ? SVO_ERR_INVALID : SVO_OK) && bytes == (c.want ? 0 : (size_t)40 << c.lg), "bytes: vs %g lg %d -> rc %d, %zu", (double)c.vs, c.lg, rc, bytes);
  }
  EXPECT(voxel_params_check(nullptr, &err), "voxel_map_create: null params", "null params");
  const svo_voxel_map_params p = {0.1f, 8, 0.0f}, q = {0.1f, 28, 0.0f};
  size_t b = 0;
  CHECK(voxel_table_bytes(&p, &b) == SVO_OK && b == 10240, "bytes at 8: %zu", b);
  CHECK(voxel_table_bytes(&q, &b) == SVO_OK && b == 10737418240ull, "bytes at 28: %zu", b);
  CHECK(voxel_table_bytes(&p, nullptr) == SVO_ERR_INVALID, "null bytes");
  b = 5;
  CHECK(voxel_table_bytes(nullptr, &b) == SVO_ERR_INVALID && b == 0, "bytes of null params");
}

static void cloud_args() {
  alignas(16) static unsigned char buf[64];
  const double m[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  const struct { const VoxelCloudTexts* t; const char *neg, *mat, *pts, *al, *cnt; } entries[] = {
      {&VOXEL_INSERT_TEXTS, "voxel_map_insert: n must not be negative", "voxel_map_insert: null m12", "voxel_map_insert: null points",
       "voxel_map_insert: points must be 4-byte aligned", "voxel_map_insert: counts must be 8-byte aligned"},
      {&VOXEL_REMOVE_TEXTS, "voxel_map_remove: n must not be negative", "voxel_map_remove: null m12", "voxel_map_remove: null points",
       "voxel_map_remove: points must be 4-byte aligned", "voxel_map_remove: counts must be 8-byte aligned"},
      {&VOXEL_MOVE_TEXTS, "voxel_map_move: n must not be negative", "voxel_map_move: null from_m12", "voxel_map_move: null points",
       "voxel_map_move: points must be 4-byte aligned", "voxel_map_move: counts must be 8-byte aligned"}};
  for (const auto& e : entries) {
    EXPECT(voxel_cloud_check(buf, -1, m, *e.t, &err), e.neg, "n = -1");
    EXPECT(voxel_cloud_check(buf, -1, nullptr, *e.t, &err), e.neg, "n = -1 comes before the null matrix");
    EXPECT(voxel_cloud_check(buf, 3, nullptr, *e.t, &err), e.mat, "null matrix");
    EXPECT(voxel_cloud_check(nullptr, 0, nullptr, *e.t, &err), e.mat, "null matrix at n = 0");
    EXPECT(voxel_cloud_check(nullptr, 0, m, *e.t, &err), nullptr, "n = 0 with null points");
    EXPECT(voxel_cloud_check(buf + 1, 0, m, *e.t, &err), nullptr, "n = 0 with misaligned points");
    EXPECT(voxel_cloud_check(nullptr, 1, m, *e.t, &err), e.pts, "null points");
    EXPECT(voxel_cloud_check(buf + 1, 1, m, *e.t, &err), e.al, "points at 1 mod 4");
    EXPECT(voxel_cloud_check(buf + 4, 1, m, *e.t, &err), nullptr, "points at 4 mod 16");
    EXPECT(voxel_cloud_check(buf, INT_MAX, m, *e.t, &err), nullptr, "n = INT_MAX");
    EXPECT(voxel_counts_check(buf + 4, *e.t, &err), e.cnt, "counts at 4 mod 8");
    EXPECT(voxel_counts_check(buf + 8, *e.t, &err), nullptr, "counts at 8 mod 16");
    EXPECT(voxel_counts_check(nullptr, *e.t, &err), nullptr, "null counts");
  }
}

static void carve_args() {
  const int16_t disp[1] = {0};
  const double m[12] = {0};
  const svo_camera_info cam = {700.0, 600.0, 180.0, 0, 0, 0, 0, 0.5};
  const int LW = 1280, LH = 400;  // the context's limits
  const char* wmsg = "voxel_map_carve: width below 2 radius + 1 or beyond the context's limit";
  const char* hmsg = "voxel_map_carve: height below 2 radius + 1 or beyond the context's limit";
  auto run = [&](svo_voxel_carve_params p, int w, int h, const svo_camera_info& c, const char* want, const char* where) {
    EXPECT(voxel_carve_check(disp, w, h, &c, m, &p, LW, LH, &err), want, where);
  };
  run({-1, 8, 0}, 64, 64, cam, "voxel_map_carve: radius outside 0..3", "radius -1");
  run({0, 8, 0}, 64, 64, cam, nullptr, "radius 0");
  run({3, 8, 0}, 64, 64, cam, nullptr, "radius 3");
  run({4, 8, 0}, 64, 64, cam, "voxel_map_carve: radius outside 0..3", "radius 4");
  run({1, -1, 0}, 64, 64, cam, "voxel_map_carve: margin16 outside 0..32767", "margin16 -1");
  run({1, 0, 0}, 64, 64, cam, nullptr, "margin16 0");
  run({1, 32767, 0}, 64, 64, cam, nullptr, "margin16 32767");
  run({1, 32768, 0}, 64, 64, cam, "voxel_map_carve: margin16 outside 0..32767", "margin16 32768");
  run({1, 8, -1}, 64, 64, cam, "voxel_map_carve: keep_count must not be negative", "keep_count -1");
  run({1, 8, 0}, 64, 64, cam, nullptr, "keep_count 0");
  for (int r = 0; r <= 3; ++r) {
    run({r, 8, 0}, 2 * r, 64, cam, wmsg, "width 2 r");
    run({r, 8, 0}, 2 * r + 1, 64, cam, nullptr, "width 2 r + 1");
    run({r, 8, 0}, 64, 2 * r, cam, hmsg, "height 2 r");
    run({r, 8, 0}, 64, 2 * r + 1, cam, nullptr, "height 2 r + 1");
  }
  run({1, 8, 0}, LW, LH, cam, nullptr, "width and height at the limit");
  run({1, 8, 0}, LW + 1, LH, cam, wmsg, "width beyond the limit");
  run({1, 8, 0}, LW, LH + 1, cam, hmsg, "height beyond the limit");
  svo_camera_info c0 = cam;
  c0.focal = 0.0;
  run({1, 8, 0}, 64, 64, c0, "voxel_map_carve: focal and baseline must not be 0", "focal 0");
  c0 = cam; c0.baseline = 0.0;
  run({1, 8, 0}, 64, 64, c0, "voxel_map_carve: focal and baseline must not be 0", "baseline 0");
  c0 = cam; c0.focal = -700.0; c0.baseline = -0.5;
  run({1, 8, 0}, 64, 64, c0, nullptr, "negative focal and baseline");
  const svo_voxel_carve_params p = {1, 8, 0};
  EXPECT(voxel_carve_check(nullptr, 64, 64, &cam, m, &p, LW, LH, &err), "voxel_map_carve: null disp16", "null disp16");
  EXPECT(voxel_carve_check(disp, 64, 64, nullptr, m, &p, LW, LH, &err), "voxel_map_carve: null cam", "null cam");
  EXPECT(voxel_carve_check(disp, 64, 64, &cam, nullptr, &p, LW, LH, &err), "voxel_map_carve: null w2c12", "null w2c12");
  EXPECT(voxel_carve_check(disp, 64, 64, &cam, m, nullptr, LW, LH, &err), "voxel_map_carve: null params", "null params");
}

static void render_args() {
  const double m[12] = {0};
  const svo_camera_info cam = {700.0, 600.0, 180.0, 0, 0, 0, 0, 0.5};
  const int LW = 1280, LH = 400;
  const char* wmsg = "voxel_map_render: width below 1 or beyond the context's limit";
  const char* hmsg = "voxel_map_render: height below 1 or beyond the context's limit";
  const char* fmsg = "voxel_map_render: focal must be finite and > 0";
  const char* bmsg = "voxel_map_render: baseline must be finite and > 0";
  auto run = [&](svo_voxel_render_params p, int w, int h, const svo_camera_info& c, const char* want, const char* where) {
    EXPECT(voxel_render_check(w, h, &c, m, &p, LW, LH, &err), want, where);
  };
  run({0, 8}, 64, 64, cam, "voxel_map_render: min_count must be at least 1", "min_count 0");
  run({1, 8}, 64, 64, cam, nullptr, "min_count 1");
  run({1, -1}, 64, 64, cam, "voxel_map_render: max_radius outside 0..16", "max_radius -1");
  run({1, 0}, 64, 64, cam, nullptr, "max_radius 0");
  run({1, 16}, 64, 64, cam, nullptr, "max_radius 16");
  run({1, 17}, 64, 64, cam, "voxel_map_render: max_radius outside 0..16", "max_radius 17");
  run({1, 8}, 0, 64, cam, wmsg, "width 0");
  run({1, 8}, 1, 64, cam, nullptr, "width 1");
  run({1, 8}, LW, LH, cam, nullptr, "width and height at the limit");
  run({1, 8}, LW + 1, 64, cam, wmsg, "width beyond the limit");
  run({1, 8}, 64, 0, cam, hmsg, "height 0");
  run({1, 8}, 64, 1, cam, nullptr, "height 1");
  run({1, 8}, 64, LH + 1, cam, hmsg, "height beyond the limit");
  const struct { double v; bool ok; } values[] = {{0.0, false}, {-1.0, false}, {NaN, false}, {Inf, false}, {DBL_MAX, true}, {DBL_MIN, true}};
  for (const auto& v : values) {
    svo_camera_info c = cam;
    c.focal = v.v;
    run({1, 8}, 64, 64, c, v.ok ? nullptr : fmsg, "focal");
    c = cam; c.baseline = v.v;
    run({1, 8}, 64, 64, c, v.ok ? nullptr : bmsg, "baseline");
  }
  const svo_voxel_render_params p = {1, 8};
  EXPECT(voxel_render_check(64, 64, nullptr, m, &p, LW, LH, &err), "voxel_map_render: null cam", "null cam");
  EXPECT(voxel_render_check(64, 64, &cam, nullptr, &p, LW, LH, &err), "voxel_map_render: null w2c12", "null w2c12");
  EXPECT(voxel_render_check(64, 64, &cam, m, nullptr, LW, LH, &err), "voxel_map_render: null params", "null params");
}

static void copy_box() {
  const float vs = 0.25f;  // exact in binary: a face of the grid is an exact double
  const int far = 1 << 21;
  int lo[3], hi[3];
  for (int i = 0; i < 6; ++i) {
    double box[6] = {-1, -1, -1, 1, 1, 1};
    box[i] = NaN;
    EXPECT(voxel_box_keys(box, vs, lo, hi, &err), "voxel_map_copy_live: box6 holds a NaN", "NaN in the box");
  }
  const double below = nextafter(0.75, 0.0), nbelow = nextafter(-0.75, -1.0);
  const double box[6] = {0.75, below, -0.75, nbelow, 0.0, -0.0};
  EXPECT(voxel_box_keys(box, vs, lo, hi, &err), nullptr, "faces");
  CHECK(lo[0] == 3 && lo[1] == 2 && lo[2] == -3 && hi[0] == -4 && hi[1] == 0 && hi[2] == 0, "faces: %d %d %d | %d %d %d", lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]);
  const double big[6] = {-1e300, -Inf, 1e300, 1e300, Inf, -1e300};
  EXPECT(voxel_box_keys(big, vs, lo, hi, &err), nullptr, "far bounds");
  CHECK(lo[0] == -far && lo[1] == -far && lo[2] == far && hi[0] == far && hi[1] == far && hi[2] == -far, "far: %d %d %d | %d %d %d", lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]);
  const double edge[6] = {-far * 0.25, -(far + 1) * 0.25, (far - 1) * 0.25, far * 0.25, (far + 1) * 0.25, 0.1};
  EXPECT(voxel_box_keys(edge, vs, lo, hi, &err), nullptr, "the clamp's own boundary");
  CHECK(lo[0] == -far && lo[1] == -far && lo[2] == far - 1 && hi[0] == far && hi[1] == far && hi[2] == 0, "edge: %d %d %d | %d %d %d", lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]);
}

// c2w o w2c as a 3 x 4 matrix: the rotation parts multiplied, the translation pushed through
static void compose(const double* a, const double* b, double* out) {
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) out[4 * r + c] = a[4 * r] * b[c] + a[4 * r + 1] * b[4 + c] + a[4 * r + 2] * b[8 + c];
    out[4 * r + 3] = (a[4 * r] * b[3] + a[4 * r + 1] * b[7] + a[4 * r + 2] * b[11]) + a[4 * r + 3];
  }
}

static void matrices() {
  const double eye[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  const double id[7] = {1, 0, 0, 0, 0, 0, 0};
  double m[12], w[12];
  voxel_pose7_to_cam_to_world(id, m);
  voxel_pose7_to_world_to_cam(id, w);
  for (int i = 0; i < 12; ++i) CHECK(m[i] == eye[i] && w[i] == eye[i], "identity, entry %d: %g %g", i, m[i], w[i]);
  const double half[7] = {0, 1, 0, 0, 1, 2, 3};  // half a turn about x: diag(1, -1, -1)
  const double want_w[12] = {1, 0, 0, 1, 0, -1, 0, 2, 0, 0, -1, 3}, want_m[12] = {1, 0, 0, -1, 0, -1, 0, 2, 0, 0, -1, 3};
  voxel_pose7_to_cam_to_world(half, m);
  voxel_pose7_to_world_to_cam(half, w);
  for (int i = 0; i < 12; ++i) CHECK(m[i] == want_m[i] && w[i] == want_w[i], "(0, 1, 0, 0), entry %d: %g %g", i, m[i], w[i]);
  // 4 ulp of the magnitude an entry is made of: 1 for a rotation entry (a sum of products of entries <= 1), |t|_1 for a translation
  const double ulp = DBL_EPSILON;
  double worst_i = 0, worst_s = 0;
  for (unsigned seed = 1; seed <= 10; ++seed) {
    std::mt19937 g(seed);
    std::normal_distribution<double> nd(0.0, 1.0);
    std::uniform_real_distribution<double> ud(-10.0, 10.0);
    double q[7], len = 0;
    for (int i = 0; i < 4; ++i) { q[i] = nd(g); len += q[i] * q[i]; }
    for (int i = 0; i < 4; ++i) q[i] /= sqrt(len);
    for (int i = 4; i < 7; ++i) q[i] = ud(g);
    const double t1 = fabs(q[4]) + fabs(q[5]) + fabs(q[6]);
    double c[12];
    voxel_pose7_to_cam_to_world(q, m);
    voxel_pose7_to_world_to_cam(q, w);
    compose(m, w, c);
    for (int i = 0; i < 12; ++i) {
      const double tol = 4 * ulp * (i % 4 == 3 ? t1 : 1.0), d = fabs(c[i] - eye[i]);
      worst_i = d / tol > worst_i ? d / tol : worst_i;
      CHECK(d <= tol, "seed %u: cam_to_world o world_to_cam, entry %d is %.17g (%.2f ulp of its scale)", seed, i, c[i], d / (tol / 4));
    }
    double q3[7], m3[12], w3[12];
    for (int i = 0; i < 7; ++i) q3[i] = i < 4 ? 3.0 * q[i] : q[i];
    voxel_pose7_to_cam_to_world(q3, m3);
    voxel_pose7_to_world_to_cam(q3, w3);
    for (int i = 0; i < 12; ++i) {
      const double tol = 4 * ulp * (i % 4 == 3 ? t1 : 1.0), dm = fabs(m3[i] - m[i]), dw = fabs(w3[i] - w[i]);
      worst_s = dm / tol > worst_s ? dm / tol : worst_s;
      CHECK(dm <= tol && dw <= tol, "seed %u: q scaled by 3, entry %d: %.17g / %.17g, %.17g / %.17g", seed, i, m3[i], m[i], w3[i], w[i]);
    }
  }
  printf("matrices: worst composition error %.2f, worst scaled-quaternion error %.2f (in units of the 4 ulp bound)\n", worst_i, worst_s);
}

static void geometry() {
  CHECK(voxel_walk_groups((size_t)1 << 8) == 1, "walk 2^8");
  CHECK(voxel_walk_groups((size_t)1 << 11) == 1, "walk 2^11");
  CHECK(voxel_walk_groups(((size_t)1 << 11) + 1) == 2, "walk 2^11 + 1");
  CHECK(voxel_walk_groups((size_t)1 << 28) == (size_t)1 << 17, "walk 2^28");
  CHECK(voxel_record_groups(1) == 1 && voxel_record_groups(256) == 1 && voxel_record_groups(257) == 2, "records 1, 256, 257");
  CHECK(voxel_record_groups(INT_MAX) == 8388608, "records INT_MAX: %zu", voxel_record_groups(INT_MAX));
  CHECK(voxel_resolve_groups(1) == 1 && voxel_resolve_groups(1023) == 1 && voxel_resolve_groups(1024) == 1 && voxel_resolve_groups(1025) == 2, "resolve 1..1025");
  CHECK(voxel_resolve_groups((size_t)16384 * 16384) == 262144, "resolve 16384 x 16384: %zu", voxel_resolve_groups((size_t)16384 * 16384));
  CHECK(voxel_resolve_groups((size_t)65536 * 65536) == 4194304, "resolve 2^32 pixels: %zu", voxel_resolve_groups((size_t)65536 * 65536));
  alignas(16) static unsigned char buf[64];
  CHECK(voxel_resolve_vector_ok(buf, buf + 8, buf + 4), "vector form at 16, 8 and 4 bytes");
  CHECK(voxel_resolve_vector_ok(buf, buf + 8, nullptr), "vector form without an image");
  CHECK(!voxel_resolve_vector_ok(buf + 8, buf, buf) && !voxel_resolve_vector_ok(buf + 4, buf, buf), "workspace off 16 bytes");
  CHECK(!voxel_resolve_vector_ok(buf, buf + 4, buf) && !voxel_resolve_vector_ok(buf, buf + 2, buf), "map off 8 bytes");
  CHECK(!voxel_resolve_vector_ok(buf, buf, buf + 2) && !voxel_resolve_vector_ok(buf, buf, buf + 1), "image off 4 bytes");
}

int main() {
  map_params();
  cloud_args();
  carve_args();
  render_args();
  copy_box();
  matrices();
  geometry();
  if (fails) { fprintf(stderr, "%d failure(s)\n", fails); return 1; }
  printf("voxel args ok\n");
  return 0;
}
