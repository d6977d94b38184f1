// The ground plan clearance's GPU-free host logic (stereo_vo_amd/host/clearance_args.h) walked on the host, under ASan + UBSan: every
// refusal at its boundary with its code and its exact message and the accepted side of each boundary, R2 at integer squares, just
// below them, at 0, at the clamp and where the quotient or the square overflows, the defaults, the workspace size past 2^32 and
// the launch geometry.
#include <limits.h>
#include <stdio.h>
#include <string.h>

#include <initializer_list>
#include <limits>

#include "clearance_args.h"

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
using P = svo_grid_clearance_params;

static P good() {
  P p;
  p.na = 32; p.nb = 13; p.source_mask = 1u << 2; p.max_dist = 64; p.cell_size = 0.5; p.inflate_radius = 0.0;
  return p;
}

template <typename F>
static void param_case(F change, const char* want, const char* where) {
  P p = good();
  change(p);
  EXPECT(clearance_params_check(&p, &err), want, where);
}

static void params() {
  const char *na = "grid_clearance: na outside 1..8192", *nb = "grid_clearance: nb outside 1..8192", *area = "grid_clearance: na * nb beyond 2^24";
  const char *mask = "grid_clearance: source_mask must not be 0", *md = "grid_clearance: max_dist outside 1..8191";
  const char *cs = "grid_clearance: cell_size must be finite and > 0", *ir = "grid_clearance: inflate_radius must be finite and >= 0";
  EXPECT(clearance_params_check(nullptr, &err), "grid_clearance: null params", "null params");
  param_case([](P&) {}, nullptr, "a good set");
  param_case([](P& p) { p.na = 0; }, na, "na 0");
  param_case([](P& p) { p.na = 1; }, nullptr, "na 1");
  param_case([](P& p) { p.na = 8192; }, nullptr, "na 8192");
  param_case([](P& p) { p.na = 8193; }, na, "na 8193");
  param_case([](P& p) { p.na = INT_MIN; }, na, "na INT_MIN");
  param_case([](P& p) { p.na = INT_MAX; }, na, "na INT_MAX");
  param_case([](P& p) { p.nb = 0; }, nb, "nb 0");
  param_case([](P& p) { p.nb = 1; }, nullptr, "nb 1");
  param_case([](P& p) { p.nb = 8192; }, nullptr, "nb 8192");
  param_case([](P& p) { p.nb = 8193; }, nb, "nb 8193");
  param_case([](P& p) { p.nb = -1; }, nb, "nb -1");
  param_case([](P& p) { p.na = 8192; p.nb = 2048; }, nullptr, "2^24 cells");
  param_case([](P& p) { p.na = 2048; p.nb = 8192; }, nullptr, "2^24 cells the other way");
  param_case([](P& p) { p.na = 8192; p.nb = 2049; }, area, "2^24 + 8192 cells");
  param_case([](P& p) { p.na = 4097; p.nb = 4096; }, area, "2^24 + 4096 cells");
  param_case([](P& p) { p.na = 8192; p.nb = 8192; }, area, "2^26 cells");
  param_case([](P& p) { p.source_mask = 0u; }, mask, "mask 0");
  param_case([](P& p) { p.source_mask = 1u; }, nullptr, "mask 1");
  param_case([](P& p) { p.source_mask = 1u << 31; }, nullptr, "mask bit 31");
  param_case([](P& p) { p.source_mask = 0xFFFFFFFFu; }, nullptr, "mask all");
  param_case([](P& p) { p.max_dist = 0; }, md, "max_dist 0");
  param_case([](P& p) { p.max_dist = -1; }, md, "max_dist -1");
  param_case([](P& p) { p.max_dist = 1; }, nullptr, "max_dist 1");
  param_case([](P& p) { p.max_dist = 8191; }, nullptr, "max_dist 8191");
  param_case([](P& p) { p.max_dist = 8192; }, md, "max_dist 8192");
  param_case([](P& p) { p.max_dist = INT_MAX; }, md, "max_dist INT_MAX");
  param_case([](P& p) { p.cell_size = 0.0; }, cs, "cell_size 0");
  param_case([](P& p) { p.cell_size = -0.5; }, cs, "cell_size negative");
  param_case([](P& p) { p.cell_size = NaN; }, cs, "cell_size NaN");
  param_case([](P& p) { p.cell_size = Inf; }, cs, "cell_size inf");
  param_case([](P& p) { p.cell_size = DBL_MAX; }, nullptr, "cell_size DBL_MAX");
  param_case([](P& p) { p.cell_size = std::numeric_limits<double>::denorm_min(); }, nullptr, "cell_size the smallest subnormal");
  param_case([](P& p) { p.inflate_radius = -std::numeric_limits<double>::denorm_min(); }, ir, "inflate_radius just below 0");
  param_case([](P& p) { p.inflate_radius = -0.0; }, nullptr, "inflate_radius -0");
  param_case([](P& p) { p.inflate_radius = NaN; }, ir, "inflate_radius NaN");
  param_case([](P& p) { p.inflate_radius = Inf; }, ir, "inflate_radius inf");
  param_case([](P& p) { p.inflate_radius = DBL_MAX; }, nullptr, "inflate_radius DBL_MAX");
  // the first failing test names the refusal
  param_case([](P& p) { p.na = 0; p.source_mask = 0; p.cell_size = NaN; }, na, "several at once");
}

static void pointers() {
  alignas(8) static unsigned char mem[64];
  const P p = good();
  svo_grid_clearance_out o{};
  o.dist2 = reinterpret_cast<uint32_t*>(mem);
  EXPECT(clearance_check(mem, &p, mem, &o, nullptr, &err), nullptr, "dist2 alone, no counts");
  EXPECT(clearance_check(nullptr, &p, mem, &o, nullptr, &err), "grid_clearance: null cls", "null cls");
  EXPECT(clearance_check(nullptr, nullptr, nullptr, nullptr, nullptr, &err), "grid_clearance: null cls", "everything null: cls first");
  EXPECT(clearance_check(mem, nullptr, mem, &o, nullptr, &err), "grid_clearance: null params", "null params");
  EXPECT(clearance_check(mem, &p, nullptr, &o, nullptr, &err), "grid_clearance: null workspace", "null workspace");
  EXPECT(clearance_check(mem, &p, mem, nullptr, nullptr, &err), "grid_clearance: null out", "null out");
  svo_grid_clearance_out none{};
  EXPECT(clearance_check(mem, &p, mem, &none, nullptr, &err), "grid_clearance: null dist2", "null dist2");
  EXPECT(clearance_check(mem + 1, &p, mem, &o, nullptr, &err), nullptr, "cls of any alignment");
  for (int k = 1; k < 4; ++k) {
    EXPECT(clearance_check(mem, &p, mem + k, &o, nullptr, &err), "grid_clearance: workspace must be 4-byte aligned", "workspace + k");
    svo_grid_clearance_out q = o;
    q.dist2 = reinterpret_cast<uint32_t*>(mem + k);
    EXPECT(clearance_check(mem, &p, mem, &q, nullptr, &err), "grid_clearance: dist2 must be 4-byte aligned", "dist2 + k");
    EXPECT(clearance_out_check(&q, false, &err), nullptr, "host dist2 of any alignment");
    q = o;
    q.nearest = reinterpret_cast<uint32_t*>(mem + k);
    EXPECT(clearance_check(mem, &p, mem, &q, nullptr, &err), "grid_clearance: nearest must be 4-byte aligned", "nearest + k");
    q = o;
    q.clearance = reinterpret_cast<float*>(mem + k);
    EXPECT(clearance_check(mem, &p, mem, &q, nullptr, &err), "grid_clearance: clearance must be 4-byte aligned", "clearance + k");
    q = o;
    q.blocked = mem + k;
    EXPECT(clearance_check(mem, &p, mem, &q, nullptr, &err), nullptr, "blocked of any alignment");
  }
  for (int k = 1; k < 8; ++k) EXPECT(clearance_check(mem, &p, mem, &o, mem + k, &err), "grid_clearance: counts must be 8-byte aligned", "counts + k");
  EXPECT(clearance_check(mem, &p, mem + 4, &o, mem + 8, &err), nullptr, "workspace + 4, counts + 8");
  svo_grid_clearance_out all{reinterpret_cast<uint32_t*>(mem), reinterpret_cast<uint32_t*>(mem + 4), reinterpret_cast<float*>(mem + 8), mem + 13};
  EXPECT(clearance_check(mem, &p, mem, &all, mem, &err), nullptr, "every output");
  EXPECT(clearance_out_check(nullptr, false, &err), "grid_clearance: null out", "host: null out");
  EXPECT(clearance_out_check(&none, false, &err), "grid_clearance: null dist2", "host: null dist2");
  // a refused parameter set is named before the workspace
  P bad = good();
  bad.max_dist = 0;
  EXPECT(clearance_check(mem, &bad, nullptr, nullptr, nullptr, &err), "grid_clearance: max_dist outside 1..8191", "parameters before the workspace");
}

static uint32_t r2(double radius, double cell, int max_dist) {
  P p = good();
  p.inflate_radius = radius; p.cell_size = cell; p.max_dist = max_dist;
  const char* err = nullptr;
  CHECK(clearance_params_check(&p, &err) == SVO_OK, "r2 of a refused set");
  return clearance_r2(&p);
}

static void radius() {
  CHECK(r2(0.0, 0.5, 64) == 0u, "radius 0");
  CHECK(r2(-0.0, 0.5, 64) == 0u, "radius -0");
  CHECK(r2(1.5, 0.5, 64) == 9u, "rc = 3: %u", r2(1.5, 0.5, 64));
  CHECK(r2(nextafter(1.5, 0.0), 0.5, 64) == 8u, "just below rc = 3: %u", r2(nextafter(1.5, 0.0), 0.5, 64));
  CHECK(r2(nextafter(1.5, 2.0), 0.5, 64) == 9u, "just above rc = 3");
  CHECK(r2(0.49, 0.5, 64) == 0u && r2(0.5, 0.5, 64) == 1u, "rc below and at 1");
  CHECK(r2(2.5, 0.5, 5) == 25u && r2(2.6, 0.5, 5) == 25u && r2(nextafter(2.5, 0.0), 0.5, 5) == 24u, "at the clamp of max_dist 5");
  CHECK(r2(1e6, 0.5, 64) == 4096u, "beyond the clamp");
  CHECK(r2(DBL_MAX, 0.5, 8191) == 8191u * 8191u, "the square overflows");
  CHECK(r2(DBL_MAX, std::numeric_limits<double>::denorm_min(), 8191) == 8191u * 8191u, "the quotient overflows");
  CHECK(r2(1.0, DBL_MAX, 1) == 0u, "the quotient underflows");
  CHECK(r2(8191.0, 1.0, 8191) == 8191u * 8191u && r2(8190.5, 1.0, 8191) == 67084290u, "the largest max_dist: %u", r2(8190.5, 1.0, 8191));
}

static void sizes_and_defaults() {
  CHECK(clearance_workspace_bytes(256, 256) == 4u * 256u * 256u && clearance_workspace_bytes(1, 1) == 4u, "workspace");
  CHECK(clearance_workspace_bytes(0, 5) == 0u && clearance_workspace_bytes(5, -1) == 0u && clearance_workspace_bytes(INT_MIN, INT_MIN) == 0u, "workspace of nothing");
  CHECK(clearance_workspace_bytes(8192, 2048) == (size_t)1 << 26, "the largest grid");
  CHECK(clearance_workspace_bytes(40000, 40000) == (size_t)6400000000ull, "past 2^32");
  CHECK(clearance_workspace_bytes(INT_MAX, INT_MAX) == 4 * (size_t)INT_MAX * (size_t)INT_MAX, "INT_MAX squared, in size_t");
  CHECK(clearance_groups(1) == 1 && clearance_groups(256) == 1 && clearance_groups(257) == 2 && clearance_groups((size_t)1 << 24) == 65536, "groups");
  CHECK(clearance_groups((size_t)5 << 32) == (size_t)5 << 24, "groups past 2^32");
  svo_voxel_grid_params g{};
  g.cell_voxels = 5; g.na = 256; g.nb = 200;
  P p{};
  CHECK(clearance_default_params(&g, 0.1f, &p) == SVO_OK, "defaults");
  CHECK(p.na == 256 && p.nb == 200 && p.source_mask == 4u && p.max_dist == 64 && p.cell_size == 5.0 * (double)0.1f && p.inflate_radius == 0.0, "the defaults' values");
  const char* err = nullptr;
  CHECK(clearance_params_check(&p, &err) == SVO_OK, "the defaults pass the check");
  CHECK(clearance_default_params(nullptr, 0.1f, &p) == SVO_ERR_INVALID && clearance_default_params(&g, 0.1f, nullptr) == SVO_ERR_INVALID, "null");
  const float bad_vs[] = {0.0f, -0.1f, std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity()};
  for (float vs : bad_vs) CHECK(clearance_default_params(&g, vs, &p) == SVO_ERR_INVALID, "voxel_size %g", (double)vs);
  for (int cv : {0, 1025}) { svo_voxel_grid_params h = g; h.cell_voxels = cv; CHECK(clearance_default_params(&h, 0.1f, &p) == SVO_ERR_INVALID, "cell_voxels %d", cv); }
  for (int n : {0, 8193}) {
    svo_voxel_grid_params h = g; h.na = n; CHECK(clearance_default_params(&h, 0.1f, &p) == SVO_ERR_INVALID, "na %d", n);
    h = g; h.nb = n; CHECK(clearance_default_params(&h, 0.1f, &p) == SVO_ERR_INVALID, "nb %d", n);
  }
  svo_voxel_grid_params h = g; h.na = 8192; h.nb = 2049;
  CHECK(clearance_default_params(&h, 0.1f, &p) == SVO_ERR_INVALID, "too many cells");
  h.nb = 2048; h.cell_voxels = 1024;
  CHECK(clearance_default_params(&h, 3.0f, &p) == SVO_OK && p.cell_size == 3072.0 && p.na == 8192 && p.nb == 2048, "the largest grid's defaults");
}

int main() {
  params();
  pointers();
  radius();
  sizes_and_defaults();
  if (fails) { fprintf(stderr, "%d failures\n", fails); return 1; }
  printf("grid clearance args ok\n");
  return 0;
}
