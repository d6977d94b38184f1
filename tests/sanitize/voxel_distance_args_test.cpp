// host/voxel_distance.h walked on a CPU under ASan + UBSan (tests/test_voxel_distance.py builds and runs it): every refusal at its
// boundary with code, message and order; R2 at integer squares, just below them, at the clamp and on overflow; the defaults, the
// sizes and the launch geometry; and, from the files named in argv (written by the test out of the Python restatement), the three
// passes in both forms and the query - the very statements the kernels compile, over a workspace of exactly the stated size that
// starts dirty - against the restatement's numbers.
// A file is a sequence of little-endian words: int32 d0 d1 d2 o0 o1 o2 max_dist n_spheres; f32 voxel size, f32 inflate_radius; u64
// volume words; per cell u16 dist2, u32 nearest, f32 clearance; u64 inflated words; 4 u64 counts; n spheres, n hit records, 6 u64.
#include <stdio.h>
#include <stdlib.h>

#include <limits>
#include <vector>

#include "voxel_distance.h"

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { ++fails; fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

static void expect(int rc, const char* err, const char* want, const char* where) {
  if (want) CHECK(rc == SVO_ERR_INVALID && err && strcmp(err, want) == 0, "%s: rc %d, message '%s', wanted '%s'", where, rc, err ? err : "(none)", want);
  else CHECK(rc == SVO_OK && err == nullptr, "%s: rc %d, message '%s', wanted acceptance", where, rc, err ? err : "(none)");
}

static const float NaNf = std::numeric_limits<float>::quiet_NaN(), Inff = std::numeric_limits<float>::infinity();
alignas(16) static char BUF[64];
static const int O3[3] = {0, 0, 0}, D3[3] = {64, 8, 8};

struct FieldArgs {
  const void *bits = BUF, *ws = BUF, *counts = BUF;
  const int* dims = D3;
  svo_voxel_distance_params prm{32, 0.0f};
  svo_voxel_distance_out out{(uint16_t*)BUF, (uint32_t*)BUF, (float*)BUF, (uint64_t*)BUF};
  bool no_prm = false, no_out = false;
};

template <typename F>
static void field(F set, const char* want, const char* where) {
  FieldArgs a;
  set(a);
  const char* err = nullptr;
  const int rc = voxel_distance_check(a.bits, a.dims, a.no_prm ? nullptr : &a.prm, a.ws, a.no_out ? nullptr : &a.out, a.counts, &err);
  expect(rc, err, want, where);
}

static void field_refusals() {
  static const int d0[3] = {64, 0, 1}, d2049[3] = {64, 1, 2049}, d96[3] = {96, 1, 1}, d31[3] = {2048, 1024, 1024}, d30[3] = {1024, 1024, 1024};
  field([](FieldArgs&) {}, nullptr, "good");
  field([](FieldArgs& a) { a.no_prm = true; }, "voxel_occupancy_distance: null params", "null params");
  field([](FieldArgs& a) { a.prm.max_dist = 0; }, "voxel_occupancy_distance: max_dist outside 1..254", "max_dist 0");
  field([](FieldArgs& a) { a.prm.max_dist = 255; }, "voxel_occupancy_distance: max_dist outside 1..254", "max_dist 255");
  field([](FieldArgs& a) { a.prm.max_dist = 1; }, nullptr, "max_dist 1");
  field([](FieldArgs& a) { a.prm.max_dist = 254; }, nullptr, "max_dist 254");
  field([](FieldArgs& a) { a.prm.inflate_radius = NaNf; }, "voxel_occupancy_distance: inflate_radius must be finite and not negative", "radius NaN");
  field([](FieldArgs& a) { a.prm.inflate_radius = Inff; }, "voxel_occupancy_distance: inflate_radius must be finite and not negative", "radius inf");
  field([](FieldArgs& a) { a.prm.inflate_radius = -1e-30f; }, "voxel_occupancy_distance: inflate_radius must be finite and not negative", "radius < 0");
  field([](FieldArgs& a) { a.prm.inflate_radius = -0.0f; }, nullptr, "radius -0");
  field([](FieldArgs& a) { a.prm.inflate_radius = FLT_MAX; }, nullptr, "radius FLT_MAX");
  field([](FieldArgs& a) { a.dims = nullptr; }, "voxel_map_occupancy: null dims", "null dims");
  field([](FieldArgs& a) { a.dims = d0; }, "voxel_map_occupancy: dims outside 1..2048", "dims 0");
  field([](FieldArgs& a) { a.dims = d2049; }, "voxel_map_occupancy: dims outside 1..2048", "dims 2049");
  field([](FieldArgs& a) { a.dims = d96; }, "voxel_map_occupancy: dims[0] must be a multiple of 64", "dims 96");
  field([](FieldArgs& a) { a.dims = d31; }, "voxel_map_occupancy: dims[0] * dims[1] * dims[2] beyond 2^30", "dims 2^31");
  field([](FieldArgs& a) { a.dims = d30; }, nullptr, "dims 2^30");
  field([](FieldArgs& a) { a.bits = nullptr; }, "voxel_map_occupancy: null bits", "null bits");
  field([](FieldArgs& a) { a.bits = BUF + 4; }, "voxel_map_occupancy: bits must be 8-byte aligned", "bits + 4");
  field([](FieldArgs& a) { a.ws = nullptr; }, "voxel_occupancy_distance: null workspace", "null workspace");
  field([](FieldArgs& a) { a.ws = BUF + 4; }, "voxel_occupancy_distance: workspace must be 8-byte aligned", "workspace + 4");
  field([](FieldArgs& a) { a.ws = BUF + 8; }, nullptr, "workspace + 8");
  field([](FieldArgs& a) { a.no_out = true; }, "voxel_occupancy_distance: null out", "null out");
  field([](FieldArgs& a) { a.out.dist2 = nullptr; }, "voxel_occupancy_distance: null dist2", "null dist2");
  field([](FieldArgs& a) { a.out.dist2 = (uint16_t*)(BUF + 1); }, "voxel_occupancy_distance: dist2 must be 2-byte aligned", "dist2 + 1");
  field([](FieldArgs& a) { a.out.dist2 = (uint16_t*)(BUF + 2); }, nullptr, "dist2 + 2");
  field([](FieldArgs& a) { a.out.nearest = (uint32_t*)(BUF + 2); }, "voxel_occupancy_distance: nearest must be 4-byte aligned", "nearest + 2");
  field([](FieldArgs& a) { a.out.clearance = (float*)(BUF + 2); }, "voxel_occupancy_distance: clearance must be 4-byte aligned", "clearance + 2");
  field([](FieldArgs& a) { a.out.inflated = (uint64_t*)(BUF + 4); }, "voxel_occupancy_distance: inflated must be 8-byte aligned", "inflated + 4");
  field([](FieldArgs& a) { a.counts = BUF + 4; }, "voxel_occupancy_distance: counts must be 8-byte aligned", "counts + 4");
  field([](FieldArgs& a) { a.out.nearest = nullptr; a.out.clearance = nullptr; a.out.inflated = nullptr; a.counts = nullptr; }, nullptr, "nothing optional");
  // the order: each pair names the earlier one
  field([](FieldArgs& a) { a.no_prm = true; a.dims = nullptr; }, "voxel_occupancy_distance: null params", "order params, dims");
  field([](FieldArgs& a) { a.prm.max_dist = 0; a.prm.inflate_radius = NaNf; }, "voxel_occupancy_distance: max_dist outside 1..254", "order max_dist, radius");
  field([](FieldArgs& a) { a.prm.inflate_radius = NaNf; a.dims = d96; }, "voxel_occupancy_distance: inflate_radius must be finite and not negative", "order radius, dims");
  field([](FieldArgs& a) { a.dims = d96; a.bits = nullptr; }, "voxel_map_occupancy: dims[0] must be a multiple of 64", "order dims, bits");
  field([](FieldArgs& a) { a.bits = BUF + 4; a.ws = nullptr; }, "voxel_map_occupancy: bits must be 8-byte aligned", "order bits, workspace");
  field([](FieldArgs& a) { a.ws = BUF + 4; a.no_out = true; }, "voxel_occupancy_distance: workspace must be 8-byte aligned", "order workspace, out");
  field([](FieldArgs& a) { a.out.dist2 = (uint16_t*)(BUF + 1); a.out.nearest = (uint32_t*)(BUF + 2); }, "voxel_occupancy_distance: dist2 must be 2-byte aligned", "order dist2, nearest");
  field([](FieldArgs& a) { a.out.nearest = (uint32_t*)(BUF + 2); a.out.clearance = (float*)(BUF + 2); }, "voxel_occupancy_distance: nearest must be 4-byte aligned", "order nearest, clearance");
  field([](FieldArgs& a) { a.out.clearance = (float*)(BUF + 2); a.out.inflated = (uint64_t*)(BUF + 4); }, "voxel_occupancy_distance: clearance must be 4-byte aligned", "order clearance, inflated");
  field([](FieldArgs& a) { a.out.inflated = (uint64_t*)(BUF + 4); a.counts = BUF + 4; }, "voxel_occupancy_distance: inflated must be 8-byte aligned", "order inflated, counts");

  // the host convenience
  svo_voxel_distance_params p{32, 0.0f};
  svo_voxel_distance_out o{(uint16_t*)(BUF + 1), nullptr, nullptr, nullptr};
  auto map = [&](int mc, const int* origin, const int* dims, const svo_voxel_distance_params* pp, const svo_voxel_distance_out* oo, const char* want, const char* where) {
    const char* err = nullptr;
    const int rc = voxel_map_distance_check(mc, origin, dims, pp, oo, &err);
    expect(rc, err, want, where);
  };
  map(1, O3, D3, &p, &o, nullptr, "map good, any alignment");
  map(0, O3, D3, &p, &o, "voxel_map_distance: min_count must be at least 1", "map min_count 0");
  map(0, O3, D3, nullptr, &o, "voxel_map_distance: min_count must be at least 1", "map order min_count, params");
  map(1, O3, D3, nullptr, &o, "voxel_occupancy_distance: null params", "map null params");
  map(1, nullptr, nullptr, &p, &o, "voxel_map_occupancy: null origin", "map null origin");
  map(1, O3, nullptr, &p, nullptr, "voxel_map_occupancy: null dims", "map null dims");
  map(1, O3, D3, &p, nullptr, "voxel_map_distance: null out", "map null out");
  o.dist2 = nullptr;
  map(1, O3, D3, &p, &o, "voxel_map_distance: null dist2", "map null dist2");
}

struct QueryArgs {
  const void *dist2 = BUF, *spheres = BUF, *hits = BUF, *counts = BUF;
  const int *origin = O3, *dims = D3;
  int n = 5;
  bool device = true;
};

template <typename F>
static void query(F set, const char* want, const char* where) {
  QueryArgs a;
  set(a);
  const char* err = nullptr;
  const int rc = voxel_distance_query_check(a.dist2, a.origin, a.dims, a.spheres, a.n, a.hits, a.counts, a.device, &err);
  expect(rc, err, want, where);
}

static void query_refusals() {
  static const int lo[3] = {-(1 << 20) - 1, 0, 0}, edge[3] = {-(1 << 20), (1 << 20) - 1, 0}, d96[3] = {96, 1, 1};
  query([](QueryArgs&) {}, nullptr, "good");
  query([](QueryArgs& a) { a.n = -1; }, "voxel_distance_query: n must not be negative", "n -1");
  query([](QueryArgs& a) { a.n = (1 << 20) + 1; }, "voxel_distance_query: n beyond 2^20", "n 2^20 + 1");
  query([](QueryArgs& a) { a.n = 1 << 20; }, nullptr, "n 2^20");
  query([](QueryArgs& a) { a.n = 0; a.spheres = nullptr; }, nullptr, "n 0 without spheres");
  query([](QueryArgs& a) { a.origin = nullptr; }, "voxel_map_occupancy: null origin", "null origin");
  query([](QueryArgs& a) { a.origin = lo; }, "voxel_map_occupancy: origin outside [-2^20, 2^20)", "origin low");
  query([](QueryArgs& a) { a.origin = edge; }, nullptr, "origin at both ends");
  query([](QueryArgs& a) { a.dims = nullptr; }, "voxel_map_occupancy: null dims", "null dims");
  query([](QueryArgs& a) { a.dims = d96; }, "voxel_map_occupancy: dims[0] must be a multiple of 64", "dims 96");
  query([](QueryArgs& a) { a.dist2 = nullptr; }, "voxel_distance_query: null dist2", "null dist2");
  query([](QueryArgs& a) { a.dist2 = BUF + 1; }, "voxel_distance_query: dist2 must be 2-byte aligned", "dist2 + 1");
  query([](QueryArgs& a) { a.hits = nullptr; }, "voxel_distance_query: null hits", "null hits");
  query([](QueryArgs& a) { a.hits = BUF + 8; }, "voxel_distance_query: hits must be 16-byte aligned", "hits + 8");
  query([](QueryArgs& a) { a.counts = BUF + 4; }, "voxel_distance_query: counts must be 8-byte aligned", "counts + 4");
  query([](QueryArgs& a) { a.counts = nullptr; }, nullptr, "no counts");
  query([](QueryArgs& a) { a.spheres = nullptr; }, "voxel_distance_query: null spheres", "null spheres");
  query([](QueryArgs& a) { a.spheres = BUF + 8; }, "voxel_distance_query: spheres must be 16-byte aligned", "spheres + 8");
  query([](QueryArgs& a) { a.device = false; a.spheres = BUF + 1; a.hits = BUF + 1; a.counts = BUF + 1; }, nullptr, "host form, any alignment");
  query([](QueryArgs& a) { a.device = false; a.dist2 = BUF + 1; }, "voxel_distance_query: dist2 must be 2-byte aligned", "host form, dist2 + 1");
  query([](QueryArgs& a) { a.n = -1; a.origin = nullptr; }, "voxel_distance_query: n must not be negative", "order n, origin");
  query([](QueryArgs& a) { a.dims = d96; a.dist2 = nullptr; }, "voxel_map_occupancy: dims[0] must be a multiple of 64", "order dims, dist2");
  query([](QueryArgs& a) { a.dist2 = BUF + 1; a.hits = nullptr; }, "voxel_distance_query: dist2 must be 2-byte aligned", "order dist2, hits");
  query([](QueryArgs& a) { a.hits = BUF + 8; a.counts = BUF + 4; }, "voxel_distance_query: hits must be 16-byte aligned", "order hits, counts");
  query([](QueryArgs& a) { a.counts = BUF + 4; a.spheres = nullptr; }, "voxel_distance_query: counts must be 8-byte aligned", "order counts, spheres");
}

static void pure() {
  // R2: §7k's pair at 0.5 per voxel, integer squares and the floats below them, the clamp, an overflow
  CHECK(voxel_distance_r2(0.0f, 0.5f, 32) == 0, "R2 of 0");
  CHECK(voxel_distance_r2(1.5f, 0.5f, 32) == 9, "R2 of 1.5 / 0.5");
  CHECK(voxel_distance_r2(nextafterf(1.5f, 0.0f), 0.5f, 32) == 8, "R2 just below 1.5 / 0.5");
  CHECK(voxel_distance_r2(0.5f, 0.5f, 32) == 1, "R2 of one voxel");
  CHECK(voxel_distance_r2(nextafterf(0.5f, 0.0f), 0.5f, 32) == 0, "R2 just below one voxel");
  CHECK(voxel_distance_r2(16.0f, 0.5f, 32) == 1024, "R2 at the clamp exactly");
  CHECK(voxel_distance_r2(nextafterf(16.0f, 0.0f), 0.5f, 32) == 1023, "R2 just below the clamp");
  CHECK(voxel_distance_r2(16.5f, 0.5f, 32) == 1024, "R2 clamped");
  CHECK(voxel_distance_r2(FLT_MAX, 1e-45f, 254) == 254 * 254, "R2 of the largest quotient");
  CHECK(voxel_distance_r2(FLT_MAX, 0.1f, 1) == 1, "R2 far beyond the clamp");
  CHECK(voxel_distance_r2(3.0f, 1.0f, 254) == 9 && voxel_distance_r2(nextafterf(3.0f, 0.0f), 1.0f, 254) == 8, "R2 at 3 voxels");

  svo_voxel_distance_params p{-1, -1.0f};
  CHECK(voxel_distance_default_params(0.1f, &p) == SVO_OK && p.max_dist == 32 && p.inflate_radius == 0.0f, "defaults");
  CHECK(voxel_distance_default_params(0.1f, nullptr) == SVO_ERR_INVALID, "defaults, null out");
  CHECK(voxel_distance_default_params(0.0f, &p) == SVO_ERR_INVALID && voxel_distance_default_params(NaNf, &p) == SVO_ERR_INVALID &&
            voxel_distance_default_params(Inff, &p) == SVO_ERR_INVALID && voxel_distance_default_params(-0.1f, &p) == SVO_ERR_INVALID,
        "defaults, bad voxel sizes");
  const char* err = nullptr;
  const int rc = voxel_distance_params_check(&p, &err);
  expect(rc, err, nullptr, "the defaults pass their own check");

  const int one[3] = {64, 1, 1}, odd[3] = {128, 9, 13}, def[3] = {512, 128, 512}, big[3] = {1024, 1024, 1024}, bad[3] = {96, 1, 1};
  size_t b = 7;
  CHECK(voxel_distance_bytes(one, &b) == SVO_OK && b == 128, "dist2 bytes (64, 1, 1)");
  CHECK(voxel_distance_bytes(def, &b) == SVO_OK && b == 67108864, "dist2 bytes of the default volume: %zu", b);
  CHECK(voxel_distance_bytes(big, &b) == SVO_OK && b == ((size_t)1 << 31), "dist2 bytes at 2^30 cells: %zu", b);
  CHECK(voxel_distance_bytes(bad, &b) == SVO_ERR_INVALID && b == 0, "dist2 bytes of refused dims");
  CHECK(voxel_distance_bytes(one, nullptr) == SVO_ERR_INVALID && voxel_distance_bytes(nullptr, &b) == SVO_ERR_INVALID, "dist2 bytes, null arguments");
  CHECK(voxel_distance_workspace_bytes(one, 0, &b) == SVO_OK && b == 192, "workspace (64, 1, 1)");
  CHECK(voxel_distance_workspace_bytes(one, 1, &b) == SVO_OK && b == 384, "workspace (64, 1, 1) with nearest");
  CHECK(voxel_distance_workspace_bytes(odd, 0, &b) == SVO_OK && b == (size_t)3 * 128 * 9 * 13, "workspace (128, 9, 13)");
  CHECK(voxel_distance_workspace_bytes(odd, 5, &b) == SVO_OK && b == (size_t)6 * 128 * 9 * 13, "workspace (128, 9, 13) with nearest");
  CHECK(voxel_distance_workspace_bytes(big, 0, &b) == SVO_OK && b == 3221225472ull, "workspace at 2^30 cells: %zu", b);
  CHECK(voxel_distance_workspace_bytes(big, 1, &b) == SVO_OK && b == 6442450944ull, "workspace at 2^30 cells with nearest: %zu", b);
  CHECK(voxel_distance_workspace_bytes(bad, 0, &b) == SVO_ERR_INVALID && b == 0, "workspace of refused dims");
  CHECK(voxel_distance_workspace_bytes(one, 0, nullptr) == SVO_ERR_INVALID, "workspace, null bytes");
  for (int nearest = 0; nearest < 2; ++nearest) {  // the second part: aligned for its type, behind the first, inside the whole
    const VoxelDistanceLayout l = voxel_distance_layout(odd, nearest != 0);
    const size_t n = voxel_distance_cells(odd);
    CHECK(l.second % 64 == 0 && l.second == (nearest ? 2 : 1) * n && l.total == l.second + (nearest ? 4 : 2) * n, "layout, nearest %d", nearest);
    CHECK(l.total <= (nearest ? 8 : 4) * n, "rule 7's bound, nearest %d", nearest);
  }
  // launch geometry
  CHECK(voxel_distance_groups(one) == 1 && voxel_distance_groups(odd) == (128 * 9 * 13 + 255) / 256 && voxel_distance_groups(def) == 131072 &&
            voxel_distance_groups(big) == 4194304,
        "groups of the passes");
  CHECK(voxel_distance_query_groups(1) == 1 && voxel_distance_query_groups(256) == 1 && voxel_distance_query_groups(257) == 2 &&
            voxel_distance_query_groups(1 << 20) == 4096,
        "groups of the query");
}

// ----------------------------------------------------------------------------- the passes over a restatement's file
template <typename T>
static bool rd(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

// The kernels' indexing around the header's per-cell functions.
template <bool NEAR>
static void run_field(const std::vector<uint64_t>& bits, const int* d, int max_dist, uint32_t r2, float vs, std::vector<uint16_t>& dist2,
                      std::vector<uint32_t>& nearest, std::vector<float>& clr, std::vector<uint64_t>& infl, uint64_t counts[4]) {
  typedef typename VoxelDistanceIn<NEAR, false>::T A;
  typedef typename VoxelDistanceIn<NEAR, true>::T B;
  const size_t n = voxel_distance_cells(d);
  const VoxelDistanceLayout lay = voxel_distance_layout(d, NEAR);
  std::vector<unsigned char> ws(lay.total, 0xA5);  // exactly rule 7's bytes, dirty
  A* a = reinterpret_cast<A*>(ws.data());
  B* b = reinterpret_cast<B*>(ws.data() + lay.second);
  const int wpr = d[0] >> 6;
  for (size_t i = 0; i < n; ++i) {
    const size_t word = i >> 6, row = word / wpr;
    const int off = voxel_distance_row(bits.data() + row * wpr, wpr, (int)(word - row * wpr), (int)(i & 63), max_dist);
    if (NEAR) a[i] = (A)off;
    else a[i] = off == VOXEL_DISTANCE_NO_OFFSET ? (A)255 : (A)(off < 0 ? -off : off);
  }
  const size_t s1 = d[0], s2 = (size_t)d[0] * d[1];
  for (size_t i = 0; i < n; ++i) {
    const int j1 = (int)(i / s1 % d[1]);
    const size_t line0 = i - j1 * s1;
    const VoxelDistanceBest r = voxel_distance_column<NEAR, false>(a + line0, s1, j1, d[1], max_dist, (uint32_t)line0, d[0]);
    if (NEAR) b[i] = (B)r.arg;
    else b[i] = r.d2 == VOXEL_DISTANCE_NONE ? (B)VOXEL_DISTANCE_NONE16 : (B)r.d2;
  }
  dist2.assign(n, 0x1234); nearest.assign(n, 0x12345678u); clr.assign(n, -1.0f); infl.assign(n / 64, 0);
  for (int c = 0; c < 4; ++c) counts[c] = 0;
  for (size_t i = 0; i < n; ++i) {
    const int j2 = (int)(i / s2);
    const size_t line0 = i - j2 * s2;
    const VoxelDistanceBest r = voxel_distance_column<NEAR, true>(b + line0, s2, j2, d[2], max_dist, (uint32_t)line0, d[0]);
    const bool none = r.d2 == VOXEL_DISTANCE_NONE;
    dist2[i] = none ? VOXEL_DISTANCE_NONE16 : (uint16_t)r.d2;
    nearest[i] = r.at;
    clr[i] = voxel_distance_clearance(r.d2, vs);
    if (r.d2 <= r2) { infl[i >> 6] |= 1ull << (i & 63); ++counts[3]; }
    ++counts[r.d2 == 0 ? 0 : (none ? 2 : 1)];
  }
}

static void run_file(const char* path) {
  FILE* f = fopen(path, "rb");
  CHECK(f, "cannot open %s", path);
  if (!f) return;
  int h[8];
  float fl[2];
  bool ok = fread(h, 4, 8, f) == 8 && fread(fl, 4, 2, f) == 2;
  const int *d = h, *o = h + 3, max_dist = h[6], ns = h[7];
  const size_t n = ok ? voxel_distance_cells(d) : 0;
  std::vector<uint64_t> bits, infl, counts, qcounts;
  std::vector<uint16_t> dist2;
  std::vector<uint32_t> nearest;
  std::vector<float> clr;
  std::vector<svo_voxel_sphere> spheres;
  std::vector<svo_voxel_sphere_hit> hits;
  ok = ok && rd(f, bits, n / 64) && rd(f, dist2, n) && rd(f, nearest, n) && rd(f, clr, n) && rd(f, infl, n / 64) && rd(f, counts, 4) &&
       rd(f, spheres, (size_t)ns) && rd(f, hits, (size_t)ns) && rd(f, qcounts, 6);
  fclose(f);
  CHECK(ok, "%s: short file", path);
  if (!ok) return;
  const uint32_t r2 = voxel_distance_r2(fl[1], fl[0], max_dist);
  for (int form = 0; form < 2; ++form) {
    std::vector<uint16_t> g2;
    std::vector<uint32_t> gn;
    std::vector<float> gc;
    std::vector<uint64_t> gi;
    uint64_t c[4];
    if (form) run_field<true>(bits, d, max_dist, r2, fl[0], g2, gn, gc, gi, c);
    else run_field<false>(bits, d, max_dist, r2, fl[0], g2, gn, gc, gi, c);
    size_t bad2 = 0, badn = 0, badc = 0, badi = 0;
    for (size_t i = 0; i < n; ++i) {
      bad2 += g2[i] != dist2[i];
      if (form) badn += gn[i] != nearest[i];
      badc += memcmp(&gc[i], &clr[i], 4) != 0;
    }
    for (size_t w = 0; w < n / 64; ++w) badi += gi[w] != infl[w];
    CHECK(!bad2 && !badn && !badc && !badi, "%s, form %d: %zu dist2, %zu nearest, %zu clearance, %zu inflated words differ", path, form, bad2, badn, badc, badi);
    CHECK(c[0] == counts[0] && c[1] == counts[1] && c[2] == counts[2] && c[3] == counts[3], "%s, form %d: counts", path, form);
  }
  uint64_t qc[6] = {(uint64_t)ns, 0, 0, 0, 0, 0};
  size_t badq = 0;
  for (int i = 0; i < ns; ++i) {
    const float s[4] = {spheres[i].x, spheres[i].y, spheres[i].z, spheres[i].radius};
    bool beyond = false;
    const svo_voxel_sphere_hit g = voxel_distance_query_one(s, fl[0], o, d, dist2.data(), &beyond);
    badq += memcmp(&g, &hits[i], sizeof(g)) != 0;
    ++qc[1 + g.code];
    qc[5] += beyond;
  }
  CHECK(!badq, "%s: %zu sphere records differ", path, badq);
  for (int c = 0; c < 6; ++c) CHECK(qc[c] == qcounts[c], "%s: query count %d: %llu, wanted %llu", path, c, (unsigned long long)qc[c], (unsigned long long)qcounts[c]);
  printf("%s: %zu cells, %d spheres\n", path, n, ns);
}

int main(int argc, char** argv) {
  static_assert(sizeof(svo_voxel_sphere) == 16 && sizeof(svo_voxel_sphere_hit) == 16 && sizeof(svo_voxel_distance_params) == 8, "record sizes");
  field_refusals();
  query_refusals();
  pure();
  for (int i = 1; i < argc; ++i) run_file(argv[i]);
  if (fails) { fprintf(stderr, "%d failures\n", fails); return 1; }
  printf("voxel distance args ok\n");
  return 0;
}
