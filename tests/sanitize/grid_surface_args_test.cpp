// The ground plan surface's GPU-free host logic (stereo_vo_amd/host/surface_args.h) walked on the host, under ASan + UBSan: every
// refusal at its boundary with its code and its exact message and the accepted side of each boundary, the order of the refusals,
// the rc * rc boundary at 226, r2, the half-width table for r2 = 0, 1, 2, 8, 225 (and every r2 against a brute-force count), D, the
// support comparison's edges, the tile and the defaults.
#include <limits.h>
#include <stdio.h>
#include <string.h>

#include <initializer_list>
#include <limits>

#include "surface_args.h"

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
using P = svo_grid_surface_params;

static const char *M_NA = "grid_surface: na outside 1..8192", *M_NB = "grid_surface: nb outside 1..8192", *M_AREA = "grid_surface: na * nb beyond 2^24",
                  *M_MASK = "grid_surface: ground_mask is 0", *M_CS = "grid_surface: cell_size must be finite and > 0",
                  *M_STEP = "grid_surface: max_step must be >= 0 and not NaN", *M_FR = "grid_surface: footprint_radius must be finite and >= 0",
                  *M_REACH = "grid_surface: footprint_radius beyond 15 cells (rc * rc >= 226)",
                  *M_RELIEF = "grid_surface: max_relief must be >= 0 and not NaN", *M_SUP = "grid_surface: min_support_256 outside 0..256";

static P good() {
  P p;
  p.na = 32; p.nb = 13; p.ground_mask = 1u << 1; p.cell_size = 0.5; p.max_step = 0.3; p.footprint_radius = 0.75; p.max_relief = 0.6;
  p.min_support_256 = 0;
  return p;
}

template <typename F>
static void param_case(F change, const char* want, const char* where) {
  P p = good();
  change(p);
  EXPECT(surface_params_check(&p, &err), want, where);
}

static void params() {
  param_case([](P&) {}, nullptr, "a good set");
  param_case([](P& p) { p.na = 0; }, M_NA, "na 0");
  param_case([](P& p) { p.na = 1; }, nullptr, "na 1");
  param_case([](P& p) { p.na = 8192; }, nullptr, "na 8192");
  param_case([](P& p) { p.na = 8193; }, M_NA, "na 8193");
  param_case([](P& p) { p.na = INT_MIN; }, M_NA, "na INT_MIN");
  param_case([](P& p) { p.na = INT_MAX; }, M_NA, "na INT_MAX");
  param_case([](P& p) { p.nb = 0; }, M_NB, "nb 0");
  param_case([](P& p) { p.nb = 1; }, nullptr, "nb 1");
  param_case([](P& p) { p.nb = 8192; }, nullptr, "nb 8192");
  param_case([](P& p) { p.nb = 8193; }, M_NB, "nb 8193");
  param_case([](P& p) { p.nb = -1; }, M_NB, "nb -1");
  param_case([](P& p) { p.na = 8192; p.nb = 2048; }, nullptr, "2^24 cells");
  param_case([](P& p) { p.na = 2048; p.nb = 8192; }, nullptr, "2^24 cells the other way");
  param_case([](P& p) { p.na = 8192; p.nb = 2049; }, M_AREA, "2^24 + 8192 cells");
  param_case([](P& p) { p.na = 4097; p.nb = 4096; }, M_AREA, "2^24 + 4096 cells");
  param_case([](P& p) { p.na = 8192; p.nb = 8192; }, M_AREA, "2^26 cells");
  param_case([](P& p) { p.ground_mask = 0u; }, M_MASK, "mask 0");
  param_case([](P& p) { p.ground_mask = 1u; }, nullptr, "mask 1");
  param_case([](P& p) { p.ground_mask = 1u << 31; }, nullptr, "mask bit 31");
  param_case([](P& p) { p.ground_mask = 0xFFFFFFFFu; }, nullptr, "mask all");
  param_case([](P& p) { p.cell_size = 0.0; }, M_CS, "cell_size 0");
  param_case([](P& p) { p.cell_size = -0.5; }, M_CS, "cell_size negative");
  param_case([](P& p) { p.cell_size = NaN; }, M_CS, "cell_size NaN");
  param_case([](P& p) { p.cell_size = Inf; }, M_CS, "cell_size inf");
  param_case([](P& p) { p.cell_size = DBL_MAX; }, nullptr, "cell_size DBL_MAX");
  param_case([](P& p) { p.cell_size = std::numeric_limits<double>::denorm_min(); p.footprint_radius = 0.0; }, nullptr, "cell_size the smallest subnormal");
  param_case([](P& p) { p.max_step = -std::numeric_limits<double>::denorm_min(); }, M_STEP, "max_step just below 0");
  param_case([](P& p) { p.max_step = -0.0; }, nullptr, "max_step -0");
  param_case([](P& p) { p.max_step = 0.0; }, nullptr, "max_step 0");
  param_case([](P& p) { p.max_step = NaN; }, M_STEP, "max_step NaN");
  param_case([](P& p) { p.max_step = -Inf; }, M_STEP, "max_step -inf");
  param_case([](P& p) { p.max_step = Inf; }, nullptr, "max_step +inf: the rule is off");
  param_case([](P& p) { p.footprint_radius = -std::numeric_limits<double>::denorm_min(); }, M_FR, "footprint_radius just below 0");
  param_case([](P& p) { p.footprint_radius = -0.0; }, nullptr, "footprint_radius -0");
  param_case([](P& p) { p.footprint_radius = 0.0; }, nullptr, "footprint_radius 0");
  param_case([](P& p) { p.footprint_radius = NaN; }, M_FR, "footprint_radius NaN");
  param_case([](P& p) { p.footprint_radius = Inf; }, M_FR, "footprint_radius inf");
  param_case([](P& p) { p.footprint_radius = DBL_MAX; }, M_REACH, "footprint_radius DBL_MAX: finite, and too far");
  param_case([](P& p) { p.footprint_radius = DBL_MAX; p.cell_size = std::numeric_limits<double>::denorm_min(); }, M_REACH, "the quotient overflows");
  param_case([](P& p) { p.max_relief = -std::numeric_limits<double>::denorm_min(); }, M_RELIEF, "max_relief just below 0");
  param_case([](P& p) { p.max_relief = 0.0; }, nullptr, "max_relief 0");
  param_case([](P& p) { p.max_relief = NaN; }, M_RELIEF, "max_relief NaN");
  param_case([](P& p) { p.max_relief = Inf; }, nullptr, "max_relief +inf: the rule is off");
  param_case([](P& p) { p.min_support_256 = -1; }, M_SUP, "min_support_256 -1");
  param_case([](P& p) { p.min_support_256 = 0; }, nullptr, "min_support_256 0");
  param_case([](P& p) { p.min_support_256 = 256; }, nullptr, "min_support_256 256");
  param_case([](P& p) { p.min_support_256 = 257; }, M_SUP, "min_support_256 257");
  param_case([](P& p) { p.min_support_256 = INT_MIN; }, M_SUP, "min_support_256 INT_MIN");
  // the first failing test names the refusal, in the order of the fields
  param_case([](P& p) { p.na = 0; p.ground_mask = 0; p.cell_size = NaN; }, M_NA, "several at once");
  param_case([](P& p) { p.ground_mask = 0; p.cell_size = NaN; p.max_step = NaN; }, M_MASK, "mask before cell_size");
  param_case([](P& p) { p.cell_size = NaN; p.max_step = NaN; }, M_CS, "cell_size before max_step");
  param_case([](P& p) { p.max_step = NaN; p.footprint_radius = NaN; }, M_STEP, "max_step before footprint_radius");
  param_case([](P& p) { p.footprint_radius = 100.0; p.max_relief = NaN; }, M_REACH, "the reach before max_relief");
  param_case([](P& p) { p.max_relief = NaN; p.min_support_256 = 300; }, M_RELIEF, "max_relief before min_support_256");
}

// rc * rc against 226, with rc = footprint_radius / 1.0
static void reach() {
  const double at = sqrt(226.0);  // the correctly rounded root; its square is 226 or a neighbour of it
  double lo = at, hi = at;
  while (lo * lo >= 226.0) lo = nextafter(lo, 0.0);
  while (hi * hi < 226.0) hi = nextafter(hi, Inf);
  CHECK(lo * lo < 226.0 && hi * hi >= 226.0 && nextafter(lo, Inf) * nextafter(lo, Inf) >= 226.0, "the boundary pair");
  param_case([&](P& p) { p.cell_size = 1.0; p.footprint_radius = lo; }, nullptr, "the last radius below the boundary");
  param_case([&](P& p) { p.cell_size = 1.0; p.footprint_radius = hi; }, M_REACH, "the first radius at the boundary");
  param_case([](P& p) { p.cell_size = 1.0; p.footprint_radius = 15.0; }, nullptr, "15 cells");
  param_case([](P& p) { p.cell_size = 1.0; p.footprint_radius = 16.0; }, M_REACH, "16 cells");
  P p = good();
  p.cell_size = 1.0;
  p.footprint_radius = lo;
  CHECK(surface_r2(&p) == 225u, "r2 just below the boundary: %u", surface_r2(&p));
  p.footprint_radius = 15.0;
  CHECK(surface_r2(&p) == 225u, "r2 at 15");
  p.footprint_radius = nextafter(15.0, 0.0);
  CHECK(surface_r2(&p) == 224u, "r2 just below 15: %u", surface_r2(&p));
  p.footprint_radius = 0.0;
  CHECK(surface_r2(&p) == 0u, "r2 at 0");
  p.footprint_radius = -0.0;
  CHECK(surface_r2(&p) == 0u, "r2 at -0");
  p.footprint_radius = nextafter(1.0, 0.0);
  CHECK(surface_r2(&p) == 0u, "r2 just below 1");
  p.footprint_radius = 1.0;
  CHECK(surface_r2(&p) == 1u, "r2 at 1");
  p.cell_size = 0.5; p.footprint_radius = 0.75;
  CHECK(surface_r2(&p) == 2u, "rc 1.5");
  p.cell_size = DBL_MAX; p.footprint_radius = 1.0;
  CHECK(surface_r2(&p) == 0u, "the quotient underflows");
}

static void pointers() {
  alignas(8) static unsigned char mem[64];
  const P p = good();
  svo_grid_surface_out o{};
  o.cls_out = mem + 32;
  const float* top = reinterpret_cast<const float*>(mem + 8);
  EXPECT(surface_check(mem, top, &p, &o, nullptr, true, &err), nullptr, "cls_out alone, no counts");
  EXPECT(surface_check(nullptr, nullptr, nullptr, nullptr, nullptr, true, &err), "grid_surface: null cls", "everything null: cls first");
  EXPECT(surface_check(mem, nullptr, nullptr, nullptr, nullptr, true, &err), "grid_surface: null top", "then top");
  EXPECT(surface_check(mem, top, nullptr, nullptr, nullptr, true, &err), "grid_surface: null params", "then params");
  EXPECT(surface_check(mem, top, &p, nullptr, nullptr, true, &err), "grid_surface: null out", "then out");
  svo_grid_surface_out none{};
  EXPECT(surface_check(mem, top, &p, &none, nullptr, true, &err), "grid_surface: null cls_out", "then cls_out");
  svo_grid_surface_out same{};
  same.cls_out = mem;
  EXPECT(surface_check(mem, top, &p, &same, nullptr, true, &err), "grid_surface: cls_out must not be cls", "cls_out == cls");
  EXPECT(surface_check(mem, top, &p, &same, nullptr, false, &err), "grid_surface: cls_out must not be cls", "cls_out == cls, host");
  same.cls_out = mem + 1;
  EXPECT(surface_check(mem, top, &p, &same, nullptr, true, &err), nullptr, "cls_out one byte on: the pointers differ (overlap is the caller's)");
  // cls_out == cls is named before a refused parameter, a refused parameter before an alignment
  P bad = good();
  bad.min_support_256 = 257;
  same.cls_out = mem;
  EXPECT(surface_check(mem, top, &bad, &same, nullptr, true, &err), "grid_surface: cls_out must not be cls", "cls_out == cls before the parameters");
  EXPECT(surface_check(mem, reinterpret_cast<const float*>(mem + 1), &bad, &o, nullptr, true, &err), M_SUP, "parameters before alignments");
  EXPECT(surface_check(mem + 1, top, &p, &o, nullptr, true, &err), nullptr, "cls of any alignment");
  for (int k = 1; k < 4; ++k) {
    EXPECT(surface_check(mem, reinterpret_cast<const float*>(mem + k), &p, &o, nullptr, true, &err), "grid_surface: top must be 4-byte aligned", "top + k");
    EXPECT(surface_check(mem, reinterpret_cast<const float*>(mem + k), &p, &o, nullptr, false, &err), nullptr, "host top of any alignment");
    svo_grid_surface_out q = o;
    q.step = reinterpret_cast<float*>(mem + k);
    EXPECT(surface_check(mem, top, &p, &q, nullptr, true, &err), "grid_surface: step must be 4-byte aligned", "step + k");
    q = o;
    q.relief = reinterpret_cast<float*>(mem + k);
    EXPECT(surface_check(mem, top, &p, &q, nullptr, true, &err), "grid_surface: relief must be 4-byte aligned", "relief + k");
    q = o;
    q.support = reinterpret_cast<uint16_t*>(mem + k);
    EXPECT(surface_check(mem, top, &p, &q, nullptr, true, &err), k & 1 ? "grid_surface: support must be 2-byte aligned" : nullptr, "support + k");
    q = o;
    q.cls_out = mem + 32 + k;
    EXPECT(surface_check(mem, top, &p, &q, nullptr, true, &err), nullptr, "cls_out of any alignment");
  }
  for (int k = 1; k < 8; ++k) EXPECT(surface_check(mem, top, &p, &o, mem + k, true, &err), "grid_surface: counts must be 8-byte aligned", "counts + k");
  for (int k = 1; k < 8; ++k) EXPECT(surface_check(mem, top, &p, &o, mem + k, false, &err), nullptr, "host counts of any alignment");
  // the alignments' order: top, step, relief, support, counts
  svo_grid_surface_out q = o;
  q.step = reinterpret_cast<float*>(mem + 1); q.relief = reinterpret_cast<float*>(mem + 1); q.support = reinterpret_cast<uint16_t*>(mem + 1);
  EXPECT(surface_check(mem, reinterpret_cast<const float*>(mem + 2), &p, &q, mem + 4, true, &err), "grid_surface: top must be 4-byte aligned", "top first");
  EXPECT(surface_check(mem, top, &p, &q, mem + 4, true, &err), "grid_surface: step must be 4-byte aligned", "then step");
  q.step = nullptr;
  EXPECT(surface_check(mem, top, &p, &q, mem + 4, true, &err), "grid_surface: relief must be 4-byte aligned", "then relief");
  q.relief = nullptr;
  EXPECT(surface_check(mem, top, &p, &q, mem + 4, true, &err), "grid_surface: support must be 2-byte aligned", "then support");
  q.support = nullptr;
  EXPECT(surface_check(mem, top, &p, &q, mem + 4, true, &err), "grid_surface: counts must be 8-byte aligned", "then counts");
  svo_grid_surface_out all{mem + 32, reinterpret_cast<float*>(mem + 12), reinterpret_cast<float*>(mem + 16), reinterpret_cast<uint16_t*>(mem + 22)};
  EXPECT(surface_check(mem, top, &p, &all, mem + 8, true, &err), nullptr, "every output");
}

static uint32_t brute_cells(uint32_t r2) {
  uint32_t n = 0;
  for (int da = -16; da <= 16; ++da)
    for (int db = -16; db <= 16; ++db) n += (uint32_t)(da * da + db * db) <= r2 ? 1u : 0u;
  return n;
}

static void table(uint32_t r2, int rw, std::initializer_list<int> want, uint32_t cells) {
  const SurfaceFootprint f = surface_footprint(r2);
  CHECK(f.r2 == r2 && f.rw == rw && f.cells == cells && (int)want.size() == 2 * rw + 1, "r2 %u: rw %d, cells %u", r2, f.rw, f.cells);
  int k = 0;
  for (int w : want) { CHECK(f.w[k] == w, "r2 %u: w[%d] = %d, wanted %d", r2, k, (int)f.w[k], w); ++k; }
  for (; k < SURFACE_ROWS + 1; ++k) CHECK(f.w[k] == 0, "r2 %u: w[%d] beyond the table is %d", r2, k, (int)f.w[k]);
}

static void footprint() {
  table(0, 0, {0}, 1);
  table(1, 1, {0, 1, 0}, 5);
  table(2, 1, {1, 1, 1}, 9);
  table(8, 2, {2, 2, 2, 2, 2}, 25);
  table(225, 15, {0, 5, 7, 9, 10, 11, 12, 12, 13, 13, 14, 14, 14, 14, 14, 15, 14, 14, 14, 14, 14, 13, 13, 12, 12, 11, 10, 9, 7, 5, 0}, 709);
  const uint32_t r2s[] = {0, 1, 2, 4, 8, 25, 225}, ds[] = {1, 5, 9, 13, 25, 81, 709};
  for (int k = 0; k < 7; ++k) CHECK(surface_footprint_cells(r2s[k]) == ds[k], "D(%u) = %u", r2s[k], surface_footprint_cells(r2s[k]));
  for (uint32_t r2 = 0; r2 <= SURFACE_MAX_R2; ++r2) {
    const SurfaceFootprint f = surface_footprint(r2);
    CHECK(f.cells == brute_cells(r2), "D(%u) = %u against the brute force's %u", r2, f.cells, brute_cells(r2));
    CHECK(f.rw * f.rw <= (int)r2 && (f.rw + 1) * (f.rw + 1) > (int)r2 && f.rw <= SURFACE_MAX_RW, "rw of %u", r2);
    for (int da = -f.rw; da <= f.rw; ++da) {
      const int w = f.w[f.rw + da];
      CHECK(da * da + w * w <= (int)r2 && da * da + (w + 1) * (w + 1) > (int)r2 && w <= f.rw, "r2 %u, row %d: half width %d", r2, da, w);
    }
  }
  CHECK(surface_footprint_cells(226) == 0u && surface_footprint_cells(0xFFFFFFFFu) == 0u, "D beyond 225");
  CHECK(surface_isqrt(0) == 0 && surface_isqrt(3) == 1 && surface_isqrt(4) == 2 && surface_isqrt(224) == 14 && surface_isqrt(225) == 15, "isqrt");
  CHECK(surface_isqrt(0xFFFFFFFFu) == 15, "isqrt stops at 15");
}

static void support() {
  // support * 256 < min_support_256 * D, strictly
  CHECK(!surface_unsupported(0, 0, 709), "the rule off: nothing is unsupported");
  CHECK(surface_unsupported(0, 1, 1) && !surface_unsupported(1, 1, 1), "one cell, any share");
  CHECK(!surface_unsupported(1, 256, 1) && surface_unsupported(0, 256, 1), "one cell, all of it");
  CHECK(surface_unsupported(708, 256, 709) && !surface_unsupported(709, 256, 709), "the largest footprint, all of it");
  CHECK(surface_unsupported(4, 128, 9) && !surface_unsupported(5, 128, 9), "half of nine: 4 * 256 < 1152 <= 5 * 256");
  CHECK(!surface_unsupported(1, 128, 2) && surface_unsupported(0, 128, 2), "equality is support enough: 256 == 128 * 2");
  CHECK(surface_unsupported(1, 128, 9), "the island: 256 < 1152");
  CHECK(!surface_unsupported(709, 256, 709) && 709u * 256u == 181504u, "the largest products stay far below 2^32");
}

static void tile_and_defaults() {
  CHECK(SURFACE_TILE_A * SURFACE_TILE_B == SURFACE_THREADS, "the tile");
  CHECK(surface_halo(0) == 1 && surface_halo(1) == 1 && surface_halo(2) == 2 && surface_halo(15) == 15, "the halo");
  CHECK(SURFACE_TILE_B + 2 * surface_halo(SURFACE_MAX_RW) <= SURFACE_LDS_STRIDE && SURFACE_TILE_A + 2 * surface_halo(SURFACE_MAX_RW) <= SURFACE_LDS_ROWS,
        "the largest window fits");
  CHECK(SURFACE_LDS_BYTES <= 65536, "the window's bytes: %zu", SURFACE_LDS_BYTES);
  CHECK(surface_tiles_a(1) == 1 && surface_tiles_a(SURFACE_TILE_A) == 1 && surface_tiles_a(SURFACE_TILE_A + 1) == 2, "tiles along a");
  CHECK(surface_tiles_b(1) == 1 && surface_tiles_b(SURFACE_TILE_B) == 1 && surface_tiles_b(SURFACE_TILE_B + 1) == 2, "tiles along b");
  CHECK(surface_tiles_a(8192) == 8192u / SURFACE_TILE_A && surface_tiles_b(8192) == 8192u / SURFACE_TILE_B, "the largest sides");
  CHECK(surface_tiles_a(4097) * surface_tiles_b(4095) >= 65536u, "a ragged grid of 2^24 cells has more than 65,536 tiles: %u", surface_tiles_a(4097) * surface_tiles_b(4095));
  CHECK(surface_groups(1) == 1 && surface_groups(SURFACE_MAX_GROUPS - 1) == SURFACE_MAX_GROUPS - 1 && surface_groups(SURFACE_MAX_GROUPS) == SURFACE_MAX_GROUPS &&
        surface_groups(SURFACE_MAX_GROUPS + 1) == SURFACE_MAX_GROUPS && surface_groups(0xFFFFFFFFu) == SURFACE_MAX_GROUPS, "the groups of a launch");
  svo_voxel_grid_params g{};
  g.cell_voxels = 5; g.na = 256; g.nb = 200; g.obstacle_step = 0.3;
  P p{};
  CHECK(surface_default_params(&g, 0.1f, &p) == SVO_OK, "defaults");
  CHECK(p.na == 256 && p.nb == 200 && p.ground_mask == 2u && p.cell_size == 5.0 * (double)0.1f && p.max_step == 0.3 && p.footprint_radius == 1.5 * p.cell_size &&
        p.max_relief == 0.6 && p.min_support_256 == 0, "the defaults' values");
  const char* err = nullptr;
  CHECK(surface_params_check(&p, &err) == SVO_OK && surface_r2(&p) == 2u, "the defaults pass the check, r2 = 2");
  CHECK(surface_default_params(nullptr, 0.1f, &p) == SVO_ERR_INVALID && surface_default_params(&g, 0.1f, nullptr) == SVO_ERR_INVALID, "null");
  const float bad_vs[] = {0.0f, -0.1f, std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity()};
  for (float vs : bad_vs) CHECK(surface_default_params(&g, vs, &p) == SVO_ERR_INVALID, "voxel_size %g", (double)vs);
  for (int cv : {0, 1025}) { svo_voxel_grid_params h = g; h.cell_voxels = cv; CHECK(surface_default_params(&h, 0.1f, &p) == SVO_ERR_INVALID, "cell_voxels %d", cv); }
  for (int n : {0, 8193}) {
    svo_voxel_grid_params h = g; h.na = n; CHECK(surface_default_params(&h, 0.1f, &p) == SVO_ERR_INVALID, "na %d", n);
    h = g; h.nb = n; CHECK(surface_default_params(&h, 0.1f, &p) == SVO_ERR_INVALID, "nb %d", n);
  }
  svo_voxel_grid_params h = g; h.na = 8192; h.nb = 2049;
  CHECK(surface_default_params(&h, 0.1f, &p) == SVO_ERR_INVALID, "too many cells");
  h = g; h.obstacle_step = NaN;
  CHECK(surface_default_params(&h, 0.1f, &p) == SVO_ERR_INVALID, "obstacle_step NaN");
  h.obstacle_step = -0.1;
  CHECK(surface_default_params(&h, 0.1f, &p) == SVO_ERR_INVALID, "obstacle_step negative");
  h.obstacle_step = Inf;
  CHECK(surface_default_params(&h, 0.1f, &p) == SVO_OK && p.max_step == Inf && p.max_relief == Inf && surface_params_check(&p, &err) == SVO_OK, "obstacle_step +inf: both rules off");
  h = g; h.na = 8192; h.nb = 2048; h.cell_voxels = 1024;
  CHECK(surface_default_params(&h, 3.0f, &p) == SVO_OK && p.cell_size == 3072.0 && p.footprint_radius == 4608.0 && surface_r2(&p) == 2u, "the largest grid's defaults");
}

int main() {
  params();
  reach();
  pointers();
  footprint();
  support();
  tile_and_defaults();
  if (fails) { fprintf(stderr, "%d failures\n", fails); return 1; }
  printf("grid surface args ok\n");
  return 0;
}
