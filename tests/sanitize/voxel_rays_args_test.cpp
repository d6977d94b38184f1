// host/voxel_rays.h walked on a CPU under ASan + UBSan (tests/test_voxel_rays.py builds and runs it): every refusal at its boundary
// with code, message and order; the sizes and the defaults; the launch geometry; and, from the files named in argv (written by the
// test out of the Python restatement), the set-up of every ray bit for bit and the records, pixels and counts of BOTH walks - the
// very statements the kernels compile - against the restatement's.
// A file is a sequence of little-endian words: int32 kind (0 rays, 1 camera), d0 d1 d2 o0 o1 o2 min_step n width height; f32 voxel
// size, f32 max_range; f64 focal cx cy baseline m[12]; u64 fine words; u64 coarse words; then for kind 0: n rays, n hit records, n
// set-ups {i64 p[3], L[3]; i32 D[3], ok}, 6 u64 counts; for kind 1: width*height i16, width*height u32, 7 u64 counts.
#include <stdio.h>
#include <stdlib.h>

#include <limits>
#include <vector>

#include "voxel_rays.h"

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { ++fails; fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

static void expect(int rc, const char* err, const char* want, const char* where) {
  if (want) CHECK(rc == SVO_ERR_INVALID && err && strcmp(err, want) == 0, "%s: rc %d, message '%s', wanted '%s'", where, rc, err ? err : "(none)", want);
  else CHECK(rc == SVO_OK && err == nullptr, "%s: rc %d, message '%s', wanted acceptance", where, rc, err ? err : "(none)");
}

static const float NaNf = std::numeric_limits<float>::quiet_NaN(), Inff = std::numeric_limits<float>::infinity();
static const double NaN = std::numeric_limits<double>::quiet_NaN(), Inf = std::numeric_limits<double>::infinity();
alignas(16) static char BUF[64];
static const int O3[3] = {0, 0, 0}, D3[3] = {64, 8, 8};

struct RaysArgs {
  const void *bits = BUF, *coarse = BUF, *rays = BUF, *hits = BUF, *counts = BUF;
  const int *origin = O3, *dims = D3;
  int n = 5, min_step = 1;
  bool device = true;
};

template <typename F>
static void rays(F set, const char* want, const char* where) {
  RaysArgs a;
  set(a);
  const char* err = nullptr;
  const int rc = voxel_rays_check(a.bits, a.coarse, a.origin, a.dims, a.rays, a.n, a.min_step, a.hits, a.counts, a.device, &err);
  expect(rc, err, want, where);
}

static void rays_refusals() {
  rays([](RaysArgs&) {}, nullptr, "good");
  rays([](RaysArgs& a) { a.n = -1; }, "voxel_occupancy_rays: n must not be negative", "n -1");
  rays([](RaysArgs& a) { a.n = (1 << 20) + 1; }, "voxel_occupancy_rays: n beyond 2^20", "n 2^20 + 1");
  rays([](RaysArgs& a) { a.n = 1 << 20; }, nullptr, "n 2^20");
  rays([](RaysArgs& a) { a.n = 0; a.rays = nullptr; }, nullptr, "n 0 without rays");
  rays([](RaysArgs& a) { a.min_step = -1; }, "voxel_occupancy_rays: min_step outside 0..255", "min_step -1");
  rays([](RaysArgs& a) { a.min_step = 256; }, "voxel_occupancy_rays: min_step outside 0..255", "min_step 256");
  rays([](RaysArgs& a) { a.min_step = 0; }, nullptr, "min_step 0");
  rays([](RaysArgs& a) { a.min_step = 255; }, nullptr, "min_step 255");
  rays([](RaysArgs& a) { a.origin = nullptr; }, "voxel_map_occupancy: null origin", "null origin");
  static const int lo[3] = {-(1 << 20) - 1, 0, 0}, hi[3] = {0, 0, 1 << 20}, edge[3] = {-(1 << 20), (1 << 20) - 1, 0};
  rays([](RaysArgs& a) { a.origin = lo; }, "voxel_map_occupancy: origin outside [-2^20, 2^20)", "origin low");
  rays([](RaysArgs& a) { a.origin = hi; }, "voxel_map_occupancy: origin outside [-2^20, 2^20)", "origin high");
  rays([](RaysArgs& a) { a.origin = edge; }, nullptr, "origin at both ends");
  rays([](RaysArgs& a) { a.dims = nullptr; }, "voxel_map_occupancy: null dims", "null dims");
  static const int d0[3] = {64, 0, 1}, d2049[3] = {64, 1, 2049}, d96[3] = {96, 1, 1}, d31[3] = {2048, 1024, 1024}, d30[3] = {1024, 1024, 1024};
  rays([](RaysArgs& a) { a.dims = d0; }, "voxel_map_occupancy: dims outside 1..2048", "dims 0");
  rays([](RaysArgs& a) { a.dims = d2049; }, "voxel_map_occupancy: dims outside 1..2048", "dims 2049");
  rays([](RaysArgs& a) { a.dims = d96; }, "voxel_map_occupancy: dims[0] must be a multiple of 64", "dims 96");
  rays([](RaysArgs& a) { a.dims = d31; }, "voxel_map_occupancy: dims[0] * dims[1] * dims[2] beyond 2^30", "dims 2^31");
  rays([](RaysArgs& a) { a.dims = d30; }, nullptr, "dims 2^30");
  rays([](RaysArgs& a) { a.bits = nullptr; }, "voxel_map_occupancy: null bits", "null bits");
  rays([](RaysArgs& a) { a.bits = BUF + 4; }, "voxel_map_occupancy: bits must be 8-byte aligned", "bits + 4");
  rays([](RaysArgs& a) { a.coarse = BUF + 4; }, "voxel_occupancy_rays: coarse must be 8-byte aligned", "coarse + 4");
  rays([](RaysArgs& a) { a.coarse = nullptr; }, nullptr, "no coarse");
  rays([](RaysArgs& a) { a.coarse = BUF + 8; }, nullptr, "coarse + 8");
  rays([](RaysArgs& a) { a.hits = nullptr; }, "voxel_occupancy_rays: null hits", "null hits");
  rays([](RaysArgs& a) { a.hits = BUF + 8; }, "voxel_occupancy_rays: hits must be 16-byte aligned", "hits + 8");
  rays([](RaysArgs& a) { a.counts = BUF + 4; }, "voxel_occupancy_rays: counts must be 8-byte aligned", "counts + 4");
  rays([](RaysArgs& a) { a.counts = nullptr; }, nullptr, "no counts");
  rays([](RaysArgs& a) { a.rays = nullptr; }, "voxel_occupancy_rays: null rays", "null rays");
  rays([](RaysArgs& a) { a.rays = BUF + 8; }, "voxel_occupancy_rays: rays must be 16-byte aligned", "rays + 8");
  // the host form asks no alignment of its arrays
  rays([](RaysArgs& a) { a.device = false; a.rays = BUF + 1; a.hits = BUF + 1; a.counts = BUF + 1; }, nullptr, "host form, any alignment");
  rays([](RaysArgs& a) { a.device = false; a.hits = nullptr; }, "voxel_occupancy_rays: null hits", "host form, null hits");
  // the order: each pair names the earlier one
  rays([](RaysArgs& a) { a.n = -1; a.min_step = 256; }, "voxel_occupancy_rays: n must not be negative", "order n, min_step");
  rays([](RaysArgs& a) { a.min_step = 256; a.origin = nullptr; }, "voxel_occupancy_rays: min_step outside 0..255", "order min_step, origin");
  rays([](RaysArgs& a) { a.dims = d96; a.bits = nullptr; }, "voxel_map_occupancy: dims[0] must be a multiple of 64", "order dims, bits");
  rays([](RaysArgs& a) { a.bits = BUF + 4; a.coarse = BUF + 4; }, "voxel_map_occupancy: bits must be 8-byte aligned", "order bits, coarse");
  rays([](RaysArgs& a) { a.coarse = BUF + 4; a.hits = nullptr; }, "voxel_occupancy_rays: coarse must be 8-byte aligned", "order coarse, hits");
  rays([](RaysArgs& a) { a.hits = BUF + 8; a.counts = BUF + 4; }, "voxel_occupancy_rays: hits must be 16-byte aligned", "order hits, counts");
  rays([](RaysArgs& a) { a.counts = BUF + 4; a.rays = nullptr; }, "voxel_occupancy_rays: counts must be 8-byte aligned", "order counts, rays");
}

static void coarse_refusals() {
  const char* err = nullptr;
  int rc = voxel_coarse_check(BUF, D3, BUF, &err);
  expect(rc, err, nullptr, "coarse good");
  err = nullptr; rc = voxel_coarse_check(BUF, nullptr, BUF, &err);
  expect(rc, err, "voxel_map_occupancy: null dims", "coarse null dims");
  err = nullptr; rc = voxel_coarse_check(nullptr, D3, BUF, &err);
  expect(rc, err, "voxel_map_occupancy: null bits", "coarse null bits");
  err = nullptr; rc = voxel_coarse_check(BUF + 4, D3, BUF, &err);
  expect(rc, err, "voxel_map_occupancy: bits must be 8-byte aligned", "coarse bits + 4");
  err = nullptr; rc = voxel_coarse_check(BUF, D3, nullptr, &err);
  expect(rc, err, "voxel_occupancy_coarse: null coarse", "null coarse");
  err = nullptr; rc = voxel_coarse_check(BUF, D3, BUF + 4, &err);
  expect(rc, err, "voxel_occupancy_coarse: coarse must be 8-byte aligned", "coarse + 4");
  err = nullptr; rc = voxel_coarse_check(nullptr, D3, nullptr, &err);
  expect(rc, err, "voxel_map_occupancy: null bits", "coarse order");
  size_t b = 7;
  CHECK(voxel_coarse_bytes(D3, &b) == SVO_OK && b == 8, "coarse bytes (64, 8, 8)");
  const int def[3] = {512, 128, 512}, odd[3] = {128, 9, 13}, big[3] = {1024, 1024, 1024}, bad[3] = {96, 1, 1};
  CHECK(voxel_coarse_bytes(def, &b) == SVO_OK && b == 8192, "coarse bytes of the default volume: %zu", b);
  CHECK(voxel_coarse_bytes(odd, &b) == SVO_OK && b == 8 && voxel_coarse_words(odd) == 1, "coarse bytes (128, 9, 13): 16 * 2 * 2 bits");
  CHECK(voxel_coarse_bytes(big, &b) == SVO_OK && b == (1u << 18), "coarse bytes 2^30");
  b = 7;
  CHECK(voxel_coarse_bytes(bad, &b) == SVO_ERR_INVALID && b == 0, "coarse bytes refuse");
  CHECK(voxel_coarse_bytes(nullptr, &b) == SVO_ERR_INVALID && voxel_coarse_bytes(D3, nullptr) == SVO_ERR_INVALID, "coarse bytes nulls");
  CHECK(voxel_coarse_groups(def) == 2048 && voxel_coarse_groups(D3) == 1, "coarse groups");
  CHECK(voxel_rays_groups(1) == 1 && voxel_rays_groups(256) == 1 && voxel_rays_groups(257) == 2 && voxel_rays_groups(1 << 20) == 4096, "ray groups");
  CHECK(voxel_raycast_groups(8, 8) == 1 && voxel_raycast_groups(9, 8) == 1 && voxel_raycast_groups(33, 8) == 2 && voxel_raycast_groups(1241, 376) == 1833, "tile groups");
}

struct CastArgs {
  svo_camera_info cam = {60.0, 31.5, 23.5, 0, 0, 0, 0, 0.5};
  svo_voxel_raycast_params prm = {30.0f, 1};
  double m[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  const svo_camera_info* camp = &cam;
  const svo_voxel_raycast_params* prmp = &prm;
  const double* mp = m;
  const void *bits = BUF, *coarse = BUF, *disp = BUF, *cell = BUF, *counts = BUF;
  const int *origin = O3, *dims = D3;
  int width = 64, height = 48;
};

template <typename F>
static void cast(F set, const char* want, const char* where) {
  CastArgs a;
  set(a);
  const char* err = nullptr;
  const int rc = voxel_raycast_check(a.bits, a.coarse, a.origin, a.dims, a.width, a.height, a.camp, a.mp, a.prmp, 1280, 720, a.disp, a.cell, a.counts, &err);
  expect(rc, err, want, where);
}

static void raycast_refusals() {
  cast([](CastArgs&) {}, nullptr, "good");
  cast([](CastArgs& a) { a.camp = nullptr; }, "voxel_occupancy_raycast: null cam", "null cam");
  cast([](CastArgs& a) { a.mp = nullptr; }, "voxel_occupancy_raycast: null c2w12", "null c2w12");
  cast([](CastArgs& a) { a.prmp = nullptr; }, "voxel_occupancy_raycast: null params", "null params");
  const char* mr = "voxel_occupancy_raycast: max_range must be finite and not negative";
  for (float bad : {-1.0f, -FLT_MIN, NaNf, Inff}) cast([bad](CastArgs& a) { a.prm.max_range = bad; }, mr, "max_range");
  for (float ok : {0.0f, FLT_MAX}) cast([ok](CastArgs& a) { a.prm.max_range = ok; }, nullptr, "max_range");
  cast([](CastArgs& a) { a.prm.min_step = -1; }, "voxel_occupancy_raycast: min_step outside 0..255", "min_step -1");
  cast([](CastArgs& a) { a.prm.min_step = 256; }, "voxel_occupancy_raycast: min_step outside 0..255", "min_step 256");
  cast([](CastArgs& a) { a.prm.min_step = 255; }, nullptr, "min_step 255");
  cast([](CastArgs& a) { a.width = 0; }, "voxel_occupancy_raycast: width below 1 or beyond the context's limit", "width 0");
  cast([](CastArgs& a) { a.width = 1281; }, "voxel_occupancy_raycast: width below 1 or beyond the context's limit", "width 1281");
  cast([](CastArgs& a) { a.width = 1280; a.height = 720; }, nullptr, "the limits");
  cast([](CastArgs& a) { a.height = 0; }, "voxel_occupancy_raycast: height below 1 or beyond the context's limit", "height 0");
  cast([](CastArgs& a) { a.height = 721; }, "voxel_occupancy_raycast: height below 1 or beyond the context's limit", "height 721");
  for (double bad : {0.0, -1.0, NaN, Inf}) {
    cast([bad](CastArgs& a) { a.cam.focal = bad; }, "voxel_occupancy_raycast: focal must be finite and > 0", "focal");
    cast([bad](CastArgs& a) { a.cam.baseline = bad; }, "voxel_occupancy_raycast: baseline must be finite and > 0", "baseline");
  }
  cast([](CastArgs& a) { a.origin = nullptr; }, "voxel_map_occupancy: null origin", "null origin");
  cast([](CastArgs& a) { a.dims = nullptr; }, "voxel_map_occupancy: null dims", "null dims");
  cast([](CastArgs& a) { a.bits = nullptr; }, "voxel_map_occupancy: null bits", "null bits");
  cast([](CastArgs& a) { a.coarse = BUF + 4; }, "voxel_occupancy_rays: coarse must be 8-byte aligned", "coarse + 4");
  cast([](CastArgs& a) { a.coarse = nullptr; }, nullptr, "no coarse");
  cast([](CastArgs& a) { a.disp = nullptr; }, "voxel_occupancy_raycast: null disp16", "null disp16");
  cast([](CastArgs& a) { a.disp = BUF + 1; }, "voxel_occupancy_raycast: disp16 must be 2-byte aligned", "disp16 + 1");
  cast([](CastArgs& a) { a.cell = BUF + 2; }, "voxel_occupancy_raycast: cell must be 4-byte aligned", "cell + 2");
  cast([](CastArgs& a) { a.cell = nullptr; a.counts = nullptr; }, nullptr, "no cell, no counts");
  cast([](CastArgs& a) { a.counts = BUF + 4; }, "voxel_occupancy_raycast: counts must be 8-byte aligned", "counts + 4");
  // the order
  cast([](CastArgs& a) { a.prm.max_range = -1.0f; a.prm.min_step = 256; }, mr, "order max_range, min_step");
  cast([](CastArgs& a) { a.prm.min_step = 256; a.width = 0; }, "voxel_occupancy_raycast: min_step outside 0..255", "order min_step, width");
  cast([](CastArgs& a) { a.height = 0; a.cam.focal = 0.0; }, "voxel_occupancy_raycast: height below 1 or beyond the context's limit", "order height, focal");
  cast([](CastArgs& a) { a.cam.baseline = 0.0; a.origin = nullptr; }, "voxel_occupancy_raycast: baseline must be finite and > 0", "order baseline, origin");
  cast([](CastArgs& a) { a.coarse = BUF + 4; a.disp = nullptr; }, "voxel_occupancy_rays: coarse must be 8-byte aligned", "order coarse, disp16");
  cast([](CastArgs& a) { a.disp = BUF + 1; a.cell = BUF + 2; }, "voxel_occupancy_raycast: disp16 must be 2-byte aligned", "order disp16, cell");
  // the host convenience
  CastArgs a;
  const char* err = nullptr;
  int rc = voxel_map_raycast_check(1, D3, 64, 48, &a.cam, a.m, &a.prm, 1280, 720, BUF + 1, &err);
  expect(rc, err, nullptr, "map_raycast good");
  err = nullptr; rc = voxel_map_raycast_check(0, nullptr, 0, 48, nullptr, a.m, &a.prm, 1280, 720, BUF, &err);
  expect(rc, err, "voxel_map_raycast: min_count must be at least 1", "map_raycast min_count first");
  err = nullptr; rc = voxel_map_raycast_check(1, nullptr, 0, 48, &a.cam, a.m, &a.prm, 1280, 720, BUF, &err);
  expect(rc, err, "voxel_occupancy_raycast: width below 1 or beyond the context's limit", "map_raycast width before dims");
  err = nullptr; rc = voxel_map_raycast_check(1, nullptr, 64, 48, &a.cam, a.m, &a.prm, 1280, 720, nullptr, &err);
  expect(rc, err, "voxel_map_occupancy: null dims", "map_raycast dims before disp16");
  err = nullptr; rc = voxel_map_raycast_check(1, D3, 64, 48, &a.cam, a.m, &a.prm, 1280, 720, nullptr, &err);
  expect(rc, err, "voxel_map_raycast: null disp16", "map_raycast null disp16");
  svo_voxel_raycast_params d = {0.0f, 0};
  CHECK(voxel_raycast_default_params(&d) == SVO_OK && d.max_range == 30.0f && d.min_step == 1, "defaults");
  CHECK(voxel_raycast_default_params(nullptr) == SVO_ERR_INVALID, "defaults refuse null");
  CHECK(sizeof(svo_voxel_ray) == 32 && sizeof(svo_voxel_ray_hit) == 16 && sizeof(svo_voxel_raycast_params) == 8, "record sizes");
}

// ----------------------------------------------------------------------------- the restatement's files
struct Reader {
  std::vector<char> data;
  size_t at = 0;
  template <typename T>
  std::vector<T> take(size_t n) {
    std::vector<T> v(n);
    if (at + n * sizeof(T) > data.size()) { fprintf(stderr, "short file\n"); exit(2); }
    if (n) memcpy(v.data(), data.data() + at, n * sizeof(T));
    at += n * sizeof(T);
    return v;
  }
};

struct SetupRow { long long p[3], L[3]; int D[3], ok; };

static void count(uint64_t* c, const VoxelRayEnd& e) { ++c[e.code]; c[5] += e.steps; }

static void file(const char* path) {
  Reader r;
  FILE* f = fopen(path, "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
  char buf[65536];
  for (size_t got; (got = fread(buf, 1, sizeof(buf), f)) > 0;) r.data.insert(r.data.end(), buf, buf + got);
  fclose(f);
  const std::vector<int> h = r.take<int>(10);
  const int kind = h[0], dims[3] = {h[1], h[2], h[3]}, origin[3] = {h[4], h[5], h[6]}, min_step = h[7], n = h[8], W = h[9];
  const int H = r.take<int>(1)[0];
  const std::vector<float> fl = r.take<float>(2);
  const float vs = fl[0], max_range = fl[1];
  r.take<int>(1);  // padding to 8 bytes
  const std::vector<double> cam = r.take<double>(16);
  const char* err = nullptr;
  CHECK(voxel_occupancy_dims_check(dims, &err) == SVO_OK, "%s: dims", path);
  const std::vector<uint64_t> bits = r.take<uint64_t>(voxel_occupancy_words(dims)), coarse = r.take<uint64_t>(voxel_coarse_words(dims));
  if (kind == 0) {
    const std::vector<svo_voxel_ray> rays = r.take<svo_voxel_ray>((size_t)n);
    const std::vector<svo_voxel_ray_hit> want = r.take<svo_voxel_ray_hit>((size_t)n);
    const std::vector<SetupRow> rows = r.take<SetupRow>((size_t)n);
    const std::vector<uint64_t> wc = r.take<uint64_t>(6);
    uint64_t c[2][6] = {{0}, {0}};
    for (int i = 0; i < n; ++i) {
      VoxelRaySetup s;
      const bool ok = voxel_ray_setup_record(rays[i], vs, origin, &s);
      CHECK(ok == (rows[i].ok != 0), "%s ray %d: ok %d", path, i, (int)ok);
      svo_voxel_ray_hit got[2];
      for (int form = 0; form < 2; ++form) {
        if (!ok) {
          got[form] = svo_voxel_ray_hit{VOXEL_RAY_NO_CELL, 0u, 0.0f, (uint32_t)VOXEL_RAY_REJECTED | 3u << 8};
          ++c[form][VOXEL_RAY_REJECTED];
          continue;
        }
        const VoxelRayEnd e = form ? voxel_ray_walk<true>(s, dims, bits.data(), coarse.data(), min_step) : voxel_ray_walk<false>(s, dims, bits.data(), nullptr, min_step);
        got[form] = voxel_ray_result(e, s, vs);
        count(c[form], e);
      }
      if (ok) {
        for (int a = 0; a < 3; ++a)
          CHECK(s.p[a] == rows[i].p[a] && s.L[a] == rows[i].L[a] && s.D[a] == rows[i].D[a], "%s ray %d axis %d: p %lld %lld L %lld %lld D %d %d", path, i, a,
                s.p[a], rows[i].p[a], s.L[a], rows[i].L[a], s.D[a], rows[i].D[a]);
      }
      for (int form = 0; form < 2; ++form)
        CHECK(memcmp(&got[form], &want[i], 16) == 0, "%s ray %d form %d: cell %u %u steps %u %u dist %a %a status %x %x", path, i, form, got[form].cell, want[i].cell,
              got[form].steps, want[i].steps, (double)got[form].dist, (double)want[i].dist, got[form].status, want[i].status);
    }
    for (int form = 0; form < 2; ++form) CHECK(memcmp(c[form], wc.data(), 48) == 0, "%s: counts of form %d", path, form);
  } else {
    const size_t px = (size_t)W * (size_t)H;
    const std::vector<int16_t> wd = r.take<int16_t>(px);
    const std::vector<uint32_t> wcell = r.take<uint32_t>(px);
    const std::vector<uint64_t> wc = r.take<uint64_t>(7);
    for (int form = 0; form < 2; ++form) {
      uint64_t c[7] = {0};
      for (int y = 0; y < H; ++y) {
        for (int x = 0; x < W; ++x) {
          double o[3], d[3];
          voxel_pixel_ray(cam.data() + 4, cam[0], cam[1], cam[2], x, y, o, d);
          VoxelRaySetup s;
          int v = -16;
          uint32_t cell = VOXEL_RAY_NO_CELL;
          if (voxel_ray_setup(o, d, (double)max_range, vs, origin, &s)) {
            const VoxelRayEnd e = form ? voxel_ray_walk<true>(s, dims, bits.data(), coarse.data(), min_step) : voxel_ray_walk<false>(s, dims, bits.data(), nullptr, min_step);
            count(c, e);
            v = voxel_ray_disp16(e, s, vs, cam[0], cam[3]);
            if (v != -16) { cell = e.cell; ++c[6]; }
          } else {
            ++c[VOXEL_RAY_REJECTED];
          }
          const size_t i = (size_t)y * (size_t)W + (size_t)x;
          CHECK(v == wd[i] && cell == wcell[i], "%s pixel (%d, %d) form %d: %d %d cell %u %u", path, x, y, form, v, (int)wd[i], cell, wcell[i]);
        }
      }
      CHECK(memcmp(c, wc.data(), 56) == 0, "%s: counts of form %d", path, form);
    }
  }
  CHECK(r.at == r.data.size(), "%s: %zu bytes left over", path, r.data.size() - r.at);
}

int main(int argc, char** argv) {
  rays_refusals();
  coarse_refusals();
  raycast_refusals();
  for (int i = 1; i < argc; ++i) file(argv[i]);
  if (fails) { fprintf(stderr, "%d failures\n", fails); return 1; }
  printf("voxel rays args ok (%d files)\n", argc - 1);
  return 0;
}
