// The voxel map grid's GPU-free host logic (stereo_vo_amd/host/voxel_args.h, the part under "the grid") walked on the host, under
// ASan + UBSan: every refusal at its boundary with its code and its exact message and the accepted side of each boundary, the three
// conversions at +-clamp, with infinite bounds and negative origins, the floor division and svo_voxel_grid_cell_of's rule at the
// grid's faces, the exact division against the 64-bit one, the defaults, the workspace size and the launch geometry.
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

static svo_voxel_grid_params good() {
  svo_voxel_grid_params p;
  p.up_axis = 1; p.up_sign = -1; p.origin_a = 0.0; p.origin_b = -3.2; p.cell_voxels = 5; p.na = 32; p.nb = 13;
  p.up_lo = -2.5; p.up_hi = 2.0; p.obstacle_step = 0.3; p.min_count = 1;
  return p;
}

template <typename F>
static void param_case(F change, const char* want, const char* where) {
  svo_voxel_grid_params p = good();
  change(p);
  EXPECT(voxel_grid_params_check(&p, &err), want, where);
}

static void params() {
  const char *axis = "voxel_map_grid: up_axis outside 0..2", *sign = "voxel_map_grid: up_sign must be +1 or -1";
  const char *oa = "voxel_map_grid: origin_a must be finite", *ob = "voxel_map_grid: origin_b must be finite";
  const char *cv = "voxel_map_grid: cell_voxels outside 1..1024", *na = "voxel_map_grid: na outside 1..8192", *nb = "voxel_map_grid: nb outside 1..8192";
  const char *area = "voxel_map_grid: na * nb beyond 2^24", *nan = "voxel_map_grid: up_lo or up_hi is a NaN", *order = "voxel_map_grid: up_lo above up_hi";
  const char *step = "voxel_map_grid: obstacle_step must not be negative or a NaN", *mc = "voxel_map_grid: min_count must be at least 1";
  EXPECT(voxel_grid_params_check(nullptr, &err), "voxel_map_grid: null params", "null params");
  param_case([](svo_voxel_grid_params&) {}, nullptr, "the street's grid");
  param_case([](svo_voxel_grid_params& p) { p.up_axis = -1; }, axis, "up_axis -1");
  param_case([](svo_voxel_grid_params& p) { p.up_axis = 0; }, nullptr, "up_axis 0");
  param_case([](svo_voxel_grid_params& p) { p.up_axis = 2; }, nullptr, "up_axis 2");
  param_case([](svo_voxel_grid_params& p) { p.up_axis = 3; }, axis, "up_axis 3");
  param_case([](svo_voxel_grid_params& p) { p.up_sign = 0; }, sign, "up_sign 0");
  param_case([](svo_voxel_grid_params& p) { p.up_sign = 1; }, nullptr, "up_sign 1");
  param_case([](svo_voxel_grid_params& p) { p.up_sign = 2; }, sign, "up_sign 2");
  param_case([](svo_voxel_grid_params& p) { p.up_sign = -2; }, sign, "up_sign -2");
  param_case([](svo_voxel_grid_params& p) { p.origin_a = NaN; }, oa, "origin_a NaN");
  param_case([](svo_voxel_grid_params& p) { p.origin_a = Inf; }, oa, "origin_a inf");
  param_case([](svo_voxel_grid_params& p) { p.origin_a = -Inf; }, oa, "origin_a -inf");
  param_case([](svo_voxel_grid_params& p) { p.origin_a = DBL_MAX; }, nullptr, "origin_a DBL_MAX");
  param_case([](svo_voxel_grid_params& p) { p.origin_a = -DBL_MAX; }, nullptr, "origin_a -DBL_MAX");
  param_case([](svo_voxel_grid_params& p) { p.origin_b = NaN; }, ob, "origin_b NaN");
  param_case([](svo_voxel_grid_params& p) { p.origin_b = -Inf; }, ob, "origin_b -inf");
  param_case([](svo_voxel_grid_params& p) { p.origin_b = DBL_MAX; }, nullptr, "origin_b DBL_MAX");
  param_case([](svo_voxel_grid_params& p) { p.cell_voxels = 0; }, cv, "cell_voxels 0");
  param_case([](svo_voxel_grid_params& p) { p.cell_voxels = 1; }, nullptr, "cell_voxels 1");
  param_case([](svo_voxel_grid_params& p) { p.cell_voxels = 1024; }, nullptr, "cell_voxels 1024");
  param_case([](svo_voxel_grid_params& p) { p.cell_voxels = 1025; }, cv, "cell_voxels 1025");
  param_case([](svo_voxel_grid_params& p) { p.na = 0; }, na, "na 0");
  param_case([](svo_voxel_grid_params& p) { p.na = 1; }, nullptr, "na 1");
  param_case([](svo_voxel_grid_params& p) { p.na = 8192; }, nullptr, "na 8192");
  param_case([](svo_voxel_grid_params& p) { p.na = 8193; }, na, "na 8193");
  param_case([](svo_voxel_grid_params& p) { p.na = INT_MIN; }, na, "na INT_MIN");
  param_case([](svo_voxel_grid_params& p) { p.nb = 0; }, nb, "nb 0");
  param_case([](svo_voxel_grid_params& p) { p.nb = 8192; }, nullptr, "nb 8192");
  param_case([](svo_voxel_grid_params& p) { p.nb = 8193; }, nb, "nb 8193");
  param_case([](svo_voxel_grid_params& p) { p.na = 8192; p.nb = 2048; }, nullptr, "2^24 cells");
  param_case([](svo_voxel_grid_params& p) { p.na = 2048; p.nb = 8192; }, nullptr, "2^24 cells the other way");
  param_case([](svo_voxel_grid_params& p) { p.na = 4096; p.nb = 4096; }, nullptr, "4096 x 4096");
  param_case([](svo_voxel_grid_params& p) { p.na = 8192; p.nb = 2049; }, area, "2^24 + 8192 cells");
  param_case([](svo_voxel_grid_params& p) { p.na = 4097; p.nb = 4096; }, area, "4097 x 4096");
  param_case([](svo_voxel_grid_params& p) { p.na = 8192; p.nb = 8192; }, area, "8192 x 8192");
  param_case([](svo_voxel_grid_params& p) { p.up_lo = NaN; }, nan, "up_lo NaN");
  param_case([](svo_voxel_grid_params& p) { p.up_hi = NaN; }, nan, "up_hi NaN");
  param_case([](svo_voxel_grid_params& p) { p.up_lo = -Inf; p.up_hi = Inf; }, nullptr, "infinite band");
  param_case([](svo_voxel_grid_params& p) { p.up_lo = Inf; p.up_hi = Inf; }, nullptr, "band at +inf");
  param_case([](svo_voxel_grid_params& p) { p.up_lo = 2.0; }, nullptr, "up_lo == up_hi");
  param_case([](svo_voxel_grid_params& p) { p.up_lo = nextafter(2.0, 3.0); }, order, "up_lo one ulp above up_hi");
  param_case([](svo_voxel_grid_params& p) { p.up_lo = Inf; p.up_hi = -Inf; }, order, "band inside out");
  param_case([](svo_voxel_grid_params& p) { p.obstacle_step = 0.0; }, nullptr, "step 0");
  param_case([](svo_voxel_grid_params& p) { p.obstacle_step = -0.0; }, nullptr, "step -0");
  param_case([](svo_voxel_grid_params& p) { p.obstacle_step = Inf; }, nullptr, "step inf");
  param_case([](svo_voxel_grid_params& p) { p.obstacle_step = -DBL_MIN; }, step, "step below 0");
  param_case([](svo_voxel_grid_params& p) { p.obstacle_step = NaN; }, step, "step NaN");
  param_case([](svo_voxel_grid_params& p) { p.min_count = 0; }, mc, "min_count 0");
  param_case([](svo_voxel_grid_params& p) { p.min_count = -5; }, mc, "min_count -5");
  param_case([](svo_voxel_grid_params& p) { p.min_count = INT_MAX; }, nullptr, "min_count INT_MAX");
}

static void pointers() {
  alignas(16) static unsigned char buf[64];
  const svo_voxel_grid_params p = good();
  svo_voxel_grid_out o = {buf, nullptr, nullptr, nullptr, nullptr, nullptr};
  EXPECT(voxel_grid_check(&p, buf, &o, nullptr, &err), nullptr, "cls alone, no counts");
  EXPECT(voxel_grid_check(nullptr, buf, &o, nullptr, &err), "voxel_map_grid: null params", "null params come first");
  EXPECT(voxel_grid_check(&p, nullptr, &o, nullptr, &err), "voxel_map_grid: null workspace", "null workspace");
  EXPECT(voxel_grid_check(&p, buf + 4, &o, nullptr, &err), "voxel_map_grid: workspace must be 8-byte aligned", "workspace at 4 mod 8");
  EXPECT(voxel_grid_check(&p, buf + 8, &o, nullptr, &err), nullptr, "workspace at 8 mod 16");
  EXPECT(voxel_grid_check(&p, buf, nullptr, nullptr, &err), "voxel_map_grid: null out", "null out");
  EXPECT(voxel_grid_check(&p, buf, &o, buf + 4, &err), "voxel_map_grid: counts must be 8-byte aligned", "counts at 4 mod 8");
  EXPECT(voxel_grid_check(&p, buf, &o, buf + 8, &err), nullptr, "counts at 8 mod 16");
  o.cls = nullptr;
  EXPECT(voxel_grid_check(&p, buf, &o, nullptr, &err), "voxel_map_grid: null cls", "null cls");
  EXPECT(voxel_grid_out_check(&o, false, &err), "voxel_map_grid: null cls", "null cls of the host entry");
  EXPECT(voxel_grid_out_check(nullptr, false, &err), "voxel_map_grid: null out", "null out of the host entry");
  o.cls = buf + 1;  // bytes: any address
  o.intensity = buf + 3;
  EXPECT(voxel_grid_out_check(&o, true, &err), nullptr, "odd byte pointers");
  const struct { int field, offset; const char* want; } cases[] = {
      {0, 2, "voxel_map_grid: top must be 4-byte aligned"}, {0, 4, nullptr}, {1, 1, "voxel_map_grid: bottom must be 4-byte aligned"}, {1, 12, nullptr},
      {2, 3, "voxel_map_grid: n_voxels must be 4-byte aligned"}, {2, 4, nullptr}, {3, 4, "voxel_map_grid: n_points must be 8-byte aligned"}, {3, 8, nullptr}};
  for (const auto& c : cases) {
    svo_voxel_grid_out q = o;
    void* at = buf + c.offset;
    if (c.field == 0) q.top = (float*)at;
    if (c.field == 1) q.bottom = (float*)at;
    if (c.field == 2) q.n_voxels = (uint32_t*)at;
    if (c.field == 3) q.n_points = (uint64_t*)at;
    EXPECT(voxel_grid_out_check(&q, true, &err), c.want, "output alignment");
    EXPECT(voxel_grid_out_check(&q, false, &err), nullptr, "the host entry asks for no alignment");
  }
}

static void conversions() {
  const long long H38 = 1ll << 38;
  svo_voxel_grid_params p = good();
  VoxelGridKeys k;
  voxel_grid_keys(&p, 0.25f, &k);  // 0.25 is exact: -3.2 / 0.25 = -12.8
  CHECK(k.ka0 == 0 && k.kb0 == -13 && k.hlo == -655360 && k.hhi == 524288 && k.step == 78643, "street at 0.25: %d %d %lld %lld %lld", k.ka0, k.kb0, k.hlo, k.hhi, k.step);
  p.origin_a = -0.25; p.origin_b = nextafter(-0.25, -1.0);  // a voxel face and one ulp below it
  voxel_grid_keys(&p, 0.25f, &k);
  CHECK(k.ka0 == -1 && k.kb0 == -2, "negative origins: %d %d", k.ka0, k.kb0);
  p.origin_a = 524288.0; p.origin_b = -524288.25;  // 2^21 voxels: the clamp's own value, and one voxel beyond the other one
  voxel_grid_keys(&p, 0.25f, &k);
  CHECK(k.ka0 == 2097152 && k.kb0 == -2097152, "at the clamp: %d %d", k.ka0, k.kb0);
  p.origin_a = 524287.75; p.origin_b = -524288.0;
  voxel_grid_keys(&p, 0.25f, &k);
  CHECK(k.ka0 == 2097151 && k.kb0 == -2097152, "inside the clamp: %d %d", k.ka0, k.kb0);
  p.origin_a = DBL_MAX; p.origin_b = -DBL_MAX;
  voxel_grid_keys(&p, FLT_MIN, &k);  // the quotient overflows to infinity
  CHECK(k.ka0 == 2097152 && k.kb0 == -2097152, "far origins: %d %d", k.ka0, k.kb0);
  p = good();
  p.up_lo = -Inf; p.up_hi = Inf; p.obstacle_step = Inf;
  voxel_grid_keys(&p, 0.1f, &k);
  CHECK(k.hlo == -H38 && k.hhi == H38 && k.step == H38, "infinite bounds: %lld %lld %lld", k.hlo, k.hhi, k.step);
  p.up_lo = -1048576.0; p.up_hi = 1048576.0; p.obstacle_step = 1048576.0;  // 2^22 voxels of 0.25: 2^38 exactly
  voxel_grid_keys(&p, 0.25f, &k);
  CHECK(k.hlo == -H38 && k.hhi == H38 && k.step == H38, "at +-2^38: %lld %lld %lld", k.hlo, k.hhi, k.step);
  p.up_lo = -1048576.25; p.up_hi = 1048575.75; p.obstacle_step = 1e30;
  voxel_grid_keys(&p, 0.25f, &k);
  CHECK(k.hlo == -H38 && k.hhi == H38 - 65536 && k.step == H38, "around +-2^38: %lld %lld %lld", k.hlo, k.hhi, k.step);
  p.up_lo = p.up_hi = -Inf; p.obstacle_step = 0.0;
  voxel_grid_keys(&p, 0.25f, &k);
  CHECK(k.hlo == -H38 && k.hhi == -H38 && k.step == 0, "a band at -inf: %lld %lld %lld", k.hlo, k.hhi, k.step);
  p.up_lo = -0.25 / 65536.0; p.up_hi = nextafter(0.25 / 65536.0, 0.0); p.obstacle_step = nextafter(0.25 / 65536.0, 0.0);  // one 65536th of a voxel
  voxel_grid_keys(&p, 0.25f, &k);
  CHECK(k.hlo == -1 && k.hhi == 0 && k.step == 0, "one unit: %lld %lld %lld", k.hlo, k.hhi, k.step);
  p.up_lo = nextafter(-0.25 / 65536.0, -1.0); p.up_hi = 0.25 / 65536.0; p.obstacle_step = 0.25 / 65536.0;
  voxel_grid_keys(&p, 0.25f, &k);
  CHECK(k.hlo == -2 && k.hhi == 1 && k.step == 1, "one unit, the other side: %lld %lld %lld", k.hlo, k.hhi, k.step);
}

static void cells() {
  const struct { int d, c, want; } fd[] = {{-1, 1, -1}, {0, 1, 0}, {-1, 5, -1}, {-5, 5, -1}, {-6, 5, -2}, {4, 5, 0}, {5, 5, 1}, {0, 1024, 0}, {-1, 1024, -1},
                                           {-3145728, 1024, -3072}, {-3145729, 1024, -3073}, {3145727, 1024, 3071}, {4194304, 1, 4194304}, {-4194304, 3, -1398102}};
  for (const auto& c : fd) CHECK(voxel_floordiv(c.d, c.c) == c.want, "floordiv(%d, %d) = %d, wanted %d", c.d, c.c, voxel_floordiv(c.d, c.c), c.want);
  svo_voxel_grid_params p = good();  // voxel 0.25: cells of 2 voxels from a = 0.25, b = -0.5, 3 x 2 of them
  p.origin_a = 0.25; p.origin_b = -0.5; p.cell_voxels = 2; p.na = 3; p.nb = 2;
  const struct { double a, b; int rc, ia, ib; } at[] = {
      {0.25, -0.5, 1, 0, 0}, {nextafter(0.25, 0.0), -0.5, 0, -1, 0}, {0.25, nextafter(-0.5, -1.0), 0, 0, -1}, {nextafter(0.75, 0.0), nextafter(0.0, -1.0), 1, 0, 0},
      {0.75, 0.0, 1, 1, 1}, {nextafter(1.75, 0.0), nextafter(0.5, 0.0), 1, 2, 1}, {1.75, 0.0, 0, 3, 1}, {1.0, 0.5, 0, 1, 2},
      {Inf, -Inf, 0, 1048575, -1048575}, {1e300, 0.0, 0, 1048575, 1}};
  for (const auto& c : at) {
    int ia = 777, ib = 777;
    const int rc = voxel_grid_cell_of(&p, 0.25f, c.a, c.b, &ia, &ib);
    CHECK(rc == c.rc && ia == c.ia && ib == c.ib, "cell_of(%g, %g) = %d (%d, %d), wanted %d (%d, %d)", c.a, c.b, rc, ia, ib, c.rc, c.ia, c.ib);
  }
  int ia = 777, ib = 777;
  CHECK(voxel_grid_cell_of(&p, 0.25f, 1.0, 0.0, nullptr, nullptr) == 1, "null ia and ib");
  CHECK(voxel_grid_cell_of(&p, 0.25f, 1.0, 0.0, &ia, nullptr) == 1 && ia == 1, "null ib");
  CHECK(voxel_grid_cell_of(&p, 0.25f, NaN, 0.0, &ia, &ib) == SVO_ERR_INVALID && voxel_grid_cell_of(&p, 0.25f, 0.0, NaN, &ia, &ib) == SVO_ERR_INVALID, "NaN position");
  CHECK(voxel_grid_cell_of(nullptr, 0.25f, 0.0, 0.0, &ia, &ib) == SVO_ERR_INVALID, "null params");
  CHECK(voxel_grid_cell_of(&p, 0.0f, 0.0, 0.0, &ia, &ib) == SVO_ERR_INVALID && voxel_grid_cell_of(&p, (float)NaN, 0.0, 0.0, &ia, &ib) == SVO_ERR_INVALID &&
            voxel_grid_cell_of(&p, (float)Inf, 0.0, 0.0, &ia, &ib) == SVO_ERR_INVALID, "voxel sizes");
  p.na = 0;
  CHECK(voxel_grid_cell_of(&p, 0.25f, 0.0, 0.0, &ia, &ib) == SVO_ERR_INVALID && ia == 1 && ib == 777, "refused params write nothing");
}

static void one_division(unsigned long long s, unsigned c) {
  const unsigned long long q = voxel_div40(s, c);
  CHECK(q == s / c, "div40(%llu, %u) = %llu, wanted %llu", s, c, q, s / c);
}

static void division() {
  const unsigned long long S = (1ull << 40) - 1;
  const unsigned cs[] = {1, 2, 3, 5, 7, 255, 256, 299, 300, 511, 512, 513, 600, 65535, 65536, 65537, (1u << 23) - 1, 1u << 23, (1u << 24) - 2, (1u << 24) - 1};
  for (unsigned c : cs) {
    const unsigned long long ss[] = {0, 1, c - 1ull, c, c + 1ull, 65535ull * c - 1, 65535ull * c, 65535ull * c + c - 1, 65536ull * c, 255ull * c + c - 1, S, S - 1, S / 2, S - c};
    for (unsigned long long s : ss) if (s <= S) one_division(s, c);
    for (unsigned long long q = 32768; q < 32768 + 4096; q += 37) {  // f32 rounds q - 1 / c up to q once c is past a few hundred
      one_division(q * c - 1, c);
      one_division(q * c, c);
    }
  }
  one_division(600ull * 40000 - 1, 600);  // the constructed voxel of tests/voxel_grid_ref.py
  one_division(599ull * 16 + 15, 600);
  std::mt19937_64 rng(20260000);
  for (int i = 0; i < 1000000; ++i) {
    const unsigned c = 1u + (unsigned)(rng() % ((1u << 24) - 1));
    const unsigned long long any = rng() & S, frac = (rng() % 65536ull) * c + rng() % c;  // any sum, and a sum a table of inserts holds
    one_division(any, c);
    one_division(frac, c);
    one_division((rng() % 65536ull) * c + (c - 1), c);  // the largest remainder
    one_division((1 + rng() % 65535ull) * c - (i & 1), c);
  }
}

static void defaults_and_geometry() {
  svo_voxel_grid_params p;
  memset(&p, 0x5A, sizeof(p));
  CHECK(voxel_grid_default_params(0.1f, &p) == SVO_OK, "defaults at 0.1");
  const double vs = (double)0.1f;
  CHECK(p.up_axis == 1 && p.up_sign == -1 && p.cell_voxels == 5 && p.na == 256 && p.nb == 256 && p.min_count == 1, "defaults: integers");
  CHECK(p.origin_a == 0.0 && p.origin_b == -128.0 * 5.0 * vs && p.up_lo == -3.0 && p.up_hi == 2.5 && p.obstacle_step == 0.3, "defaults: doubles");
  EXPECT(voxel_grid_params_check(&p, &err), nullptr, "the defaults pass their own check");
  const struct { float vs; int cv; } sizes[] = {{0.05f, 10}, {0.25f, 2}, {0.5f, 1}, {1.0f, 1}, {100.0f, 1}, {FLT_MAX, 1}, {1e-3f, 500}, {4.8828125e-4f, 1024}, {1e-6f, 1024}, {FLT_MIN, 1024}};
  for (const auto& s : sizes) {
    CHECK(voxel_grid_default_params(s.vs, &p) == SVO_OK && p.cell_voxels == s.cv, "cell_voxels at %g: %d, wanted %d", (double)s.vs, p.cell_voxels, s.cv);
    EXPECT(voxel_grid_params_check(&p, &err), nullptr, "defaults of any voxel size pass the check");
  }
  const float bad[] = {0.0f, -0.1f, (float)NaN, (float)Inf, -(float)Inf};
  for (float v : bad) CHECK(voxel_grid_default_params(v, &p) == SVO_ERR_INVALID, "defaults at %g", (double)v);
  CHECK(voxel_grid_default_params(0.1f, nullptr) == SVO_ERR_INVALID, "defaults into null");
  CHECK(voxel_grid_workspace_bytes(1, 1) == 32 && voxel_grid_workspace_bytes(32, 13) == 13312 && voxel_grid_workspace_bytes(8192, 2048) == 536870912ull, "workspace bytes");
  CHECK(voxel_grid_workspace_bytes(0, 5) == 0 && voxel_grid_workspace_bytes(5, 0) == 0 && voxel_grid_workspace_bytes(-1, -1) == 0 && voxel_grid_workspace_bytes(INT_MIN, 5) == 0, "no cells");
  CHECK(voxel_grid_workspace_bytes(40000, 40000) == 51200000000ull, "past 2^32");
  CHECK(voxel_grid_resolve_groups(1) == 1 && voxel_grid_resolve_groups(256) == 1 && voxel_grid_resolve_groups(257) == 2 && voxel_grid_resolve_groups(35) == 1 &&
            voxel_grid_resolve_groups((size_t)1 << 24) == 65536, "resolve groups");
  CHECK(voxel_walk_groups(256) == 1 && voxel_walk_groups(2048) == 1 && voxel_walk_groups(2049) == 2 && voxel_walk_groups((size_t)1 << 28) == 131072, "walk groups");
}

int main() {
  params();
  pointers();
  conversions();
  cells();
  division();
  defaults_and_geometry();
  if (fails) { fprintf(stderr, "%d checks failed\n", fails); return 1; }
  printf("voxel grid args ok\n");
  return 0;
}
