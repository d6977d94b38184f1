// The ground plan route's GPU-free host logic (stereo_vo_amd/host/route_args.h) walked on the host, under ASan + UBSan: every refusal
// at its boundary with its code and its exact message and the accepted side of each boundary, the order of the refusals, the
// workspace's size and layout, the tile count and the launch geometry at 1 x 1, T - 1, T, T + 1, 8192 x 2048 and past 2^32, the defaults.
#include <limits.h>
#include <stdio.h>
#include <string.h>

#include <initializer_list>

#include "route_args.h"

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { ++fails; fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

// rc is the refusal with exactly this message, or (want == nullptr) SVO_OK with the message untouched
static void expect(int rc, const char* err, const char* want, const char* where) {
  if (want) CHECK(rc == SVO_ERR_INVALID && err && strcmp(err, want) == 0, "%s: rc %d, message '%s', wanted '%s'", where, rc, err ? err : "(none)", want);
  else CHECK(rc == SVO_OK && err == nullptr, "%s: rc %d, message '%s', wanted acceptance", where, rc, err ? err : "(none)");
}

// the check runs first: its message is read only after it returned
#define EXPECT(call, want, where) do { const char* err = nullptr; const int rc_ = (call); expect(rc_, err, want, where); } while (0)

using P = svo_grid_route_params;
using O = svo_grid_route_out;
constexpr int T = ROUTE_TILE;

static P good() {
  P p;
  p.na = 32; p.nb = 13; p.near_r2 = 16; p.near_weight = 3; p.max_cost = 0x7F000000u; p.max_rounds = 64; p.max_path = 4096; p.resume = 0;
  return p;
}

template <typename F>
static void param_case(F change, const char* want, const char* where, int n_starts = 1) {
  P p = good();
  change(p);
  EXPECT(route_params_check(&p, n_starts, &err), want, where);
}

static void params() {
  const char *na = "grid_route: na outside 1..8192", *nb = "grid_route: nb outside 1..8192", *area = "grid_route: na * nb beyond 2^24";
  const char *r2 = "grid_route: near_r2 beyond 2^26", *pen = "grid_route: near_weight * near_r2 beyond 2^20";
  const char *mc = "grid_route: max_cost outside 1..0x7F000000", *mr = "grid_route: max_rounds outside 1..4096";
  const char *mp = "grid_route: max_path outside 1..2^20", *rs = "grid_route: resume must be 0 or 1";
  EXPECT(route_params_check(nullptr, 0, &err), "grid_route: null params", "null params");
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
  param_case([](P& p) { p.near_r2 = 0; p.near_weight = 0xFFFFFFFFu; }, nullptr, "near_r2 0 under any weight");
  param_case([](P& p) { p.near_r2 = 1u << 26; p.near_weight = 0; }, nullptr, "near_r2 2^26");
  param_case([](P& p) { p.near_r2 = (1u << 26) + 1; p.near_weight = 0; }, r2, "near_r2 2^26 + 1");
  param_case([](P& p) { p.near_r2 = 0xFFFFFFFFu; p.near_weight = 0; }, r2, "near_r2 all ones");
  param_case([](P& p) { p.near_r2 = 1u << 10; p.near_weight = 1u << 10; }, nullptr, "a penalty of 2^20");
  param_case([](P& p) { p.near_r2 = 1u << 10; p.near_weight = (1u << 10) + 1; }, pen, "a penalty of 2^20 + 2^10");
  param_case([](P& p) { p.near_r2 = 1; p.near_weight = 1u << 20; }, nullptr, "weight 2^20 at r2 1");
  param_case([](P& p) { p.near_r2 = 1; p.near_weight = (1u << 20) + 1; }, pen, "weight 2^20 + 1 at r2 1");
  param_case([](P& p) { p.near_r2 = 1u << 26; p.near_weight = 1u << 6; }, pen, "a product of 2^32: no 32-bit wrap to 0");
  param_case([](P& p) { p.near_r2 = 3; p.near_weight = 0xFFFFFFFFu; }, pen, "the largest weight");
  param_case([](P& p) { p.max_cost = 0; }, mc, "max_cost 0");
  param_case([](P& p) { p.max_cost = 1; }, nullptr, "max_cost 1");
  param_case([](P& p) { p.max_cost = 0x7F000000u; }, nullptr, "max_cost 0x7F000000");
  param_case([](P& p) { p.max_cost = 0x7F000001u; }, mc, "max_cost 0x7F000001");
  param_case([](P& p) { p.max_cost = 0xFFFFFFFFu; }, mc, "max_cost NONE");
  param_case([](P& p) { p.max_rounds = 0; }, mr, "max_rounds 0");
  param_case([](P& p) { p.max_rounds = -1; }, mr, "max_rounds -1");
  param_case([](P& p) { p.max_rounds = 1; }, nullptr, "max_rounds 1");
  param_case([](P& p) { p.max_rounds = 4096; }, nullptr, "max_rounds 4096");
  param_case([](P& p) { p.max_rounds = 4097; }, mr, "max_rounds 4097");
  param_case([](P& p) { p.max_rounds = INT_MAX; }, mr, "max_rounds INT_MAX");
  param_case([](P& p) { p.max_path = 0; }, mp, "max_path 0");
  param_case([](P& p) { p.max_path = 1; }, nullptr, "max_path 1");
  param_case([](P& p) { p.max_path = 1 << 20; }, nullptr, "max_path 2^20");
  param_case([](P& p) { p.max_path = (1 << 20) + 1; }, mp, "max_path 2^20 + 1");
  param_case([](P& p) { p.max_path = INT_MIN; }, mp, "max_path INT_MIN");
  param_case([](P& p) { p.max_path = 0; }, nullptr, "max_path 0 without starts", 0);
  param_case([](P& p) { p.max_path = INT_MAX; }, nullptr, "max_path INT_MAX without starts", 0);
  param_case([](P& p) { p.resume = 1; }, nullptr, "resume 1");
  param_case([](P& p) { p.resume = 2; }, rs, "resume 2");
  param_case([](P& p) { p.resume = -1; }, rs, "resume -1");
  // the first failing test names the refusal
  param_case([](P& p) { p.na = 0; p.max_cost = 0; p.resume = 7; }, na, "several at once");
  param_case([](P& p) { p.max_cost = 0; p.max_rounds = 0; }, mc, "max_cost before max_rounds");
  param_case([](P& p) { p.max_path = 0; p.resume = 7; }, mp, "max_path before resume");
}

static void pointers() {
  alignas(8) static unsigned char mem[64];
  const P p = good();
  O o{};
  o.cost = reinterpret_cast<uint32_t*>(mem);
  O all{reinterpret_cast<uint32_t*>(mem), mem + 1, reinterpret_cast<uint32_t*>(mem + 4), reinterpret_cast<uint32_t*>(mem + 8), mem + 13};
  auto check = [&](const void* blocked, const void* dist2, const P* prm, const void* goals, int ng, const void* starts, int ns, const void* ws,
                   const O* out, const void* counts, const char** err) { return route_check(blocked, dist2, prm, goals, ng, starts, ns, ws, out, counts, err); };
  EXPECT(check(mem, nullptr, &p, mem, 1, nullptr, 0, mem, &o, nullptr, &err), nullptr, "cost alone, no dist2, no starts, no counts");
  EXPECT(check(mem + 1, mem + 4, &p, mem, 65536, mem + 8, 4096, mem + 8, &all, mem + 16, &err), nullptr, "everything, the largest lists");
  EXPECT(check(nullptr, nullptr, nullptr, nullptr, 0, nullptr, -1, nullptr, nullptr, nullptr, &err), "grid_route: null blocked", "everything null: blocked first");
  EXPECT(check(mem, nullptr, nullptr, nullptr, 0, nullptr, -1, nullptr, nullptr, nullptr, &err), "grid_route: null params", "then params");
  EXPECT(check(mem, nullptr, &p, nullptr, 0, nullptr, -1, nullptr, nullptr, nullptr, &err), "grid_route: null goals", "then goals");
  EXPECT(check(mem, nullptr, &p, mem, 0, nullptr, -1, nullptr, nullptr, nullptr, &err), "grid_route: n_goals outside 1..65536", "then n_goals");
  EXPECT(check(mem, nullptr, &p, mem, 65537, nullptr, 0, mem, &o, nullptr, &err), "grid_route: n_goals outside 1..65536", "n_goals 65537");
  EXPECT(check(mem, nullptr, &p, mem, INT_MIN, nullptr, 0, mem, &o, nullptr, &err), "grid_route: n_goals outside 1..65536", "n_goals INT_MIN");
  EXPECT(check(mem, nullptr, &p, mem, 1, nullptr, -1, nullptr, nullptr, nullptr, &err), "grid_route: n_starts outside 0..4096", "then n_starts");
  EXPECT(check(mem, nullptr, &p, mem, 1, mem, 4097, mem, &all, nullptr, &err), "grid_route: n_starts outside 0..4096", "n_starts 4097");
  EXPECT(check(mem, nullptr, &p, mem, 1, nullptr, 1, nullptr, nullptr, nullptr, &err), "grid_route: null starts with n_starts > 0", "then starts");
  EXPECT(check(mem, nullptr, &p, mem, 1, mem, 0, mem, &o, nullptr, &err), nullptr, "starts given with n_starts 0");
  EXPECT(check(mem, nullptr, &p, mem, 1, mem, 1, nullptr, nullptr, nullptr, &err), "grid_route: null workspace", "then the workspace");
  EXPECT(check(mem, nullptr, &p, mem, 1, mem, 1, mem, nullptr, nullptr, &err), "grid_route: null out", "then out");
  O none{};
  EXPECT(check(mem, nullptr, &p, mem, 1, mem, 1, mem, &none, nullptr, &err), "grid_route: null cost", "then cost");
  const char* together = "grid_route: path, path_len and path_status go together";
  for (int miss = 1; miss < 7; ++miss) {  // every proper, non-empty subset of the three left out
    O q = all;
    if (miss & 1) q.path = nullptr;
    if (miss & 2) q.path_len = nullptr;
    if (miss & 4) q.path_status = nullptr;
    EXPECT(check(mem, nullptr, &p, mem, 1, mem, 1, mem, &q, nullptr, &err), together, "a part of the path outputs");
    EXPECT(route_out_check(&q, 1, false, &err), together, "host: a part of the path outputs");
  }
  EXPECT(check(mem, nullptr, &p, mem, 1, nullptr, 0, mem, &all, nullptr, &err), "grid_route: path outputs with n_starts == 0", "path outputs without starts");
  EXPECT(check(mem, nullptr, &p, mem, 1, mem, 3, mem, &o, nullptr, &err), nullptr, "starts without path outputs");
  P bad = good();
  bad.max_path = 0;
  EXPECT(check(mem, nullptr, &bad, mem, 1, mem, 1, mem, &all, nullptr, &err), "grid_route: max_path outside 1..2^20", "max_path with starts");
  EXPECT(check(mem, nullptr, &bad, mem, 1, nullptr, 0, mem, &o, nullptr, &err), nullptr, "max_path is not read without starts");
  for (int k = 1; k < 4; ++k) {
    O q = all;
    q.cost = reinterpret_cast<uint32_t*>(mem + k);
    EXPECT(check(mem, nullptr, &p, mem, 1, mem, 1, mem, &q, nullptr, &err), "grid_route: cost must be 4-byte aligned", "cost + k");
    EXPECT(route_out_check(&q, 1, false, &err), nullptr, "host cost of any alignment");
    q = all;
    q.path = reinterpret_cast<uint32_t*>(mem + k);
    EXPECT(check(mem, nullptr, &p, mem, 1, mem, 1, mem, &q, nullptr, &err), "grid_route: path must be 4-byte aligned", "path + k");
    q = all;
    q.path_len = reinterpret_cast<uint32_t*>(mem + k);
    EXPECT(check(mem, nullptr, &p, mem, 1, mem, 1, mem, &q, nullptr, &err), "grid_route: path_len must be 4-byte aligned", "path_len + k");
    q = all;
    q.next = mem + k; q.path_status = mem + k;
    EXPECT(check(mem + k, nullptr, &p, mem, 1, mem, 1, mem, &q, nullptr, &err), nullptr, "blocked, next and path_status of any alignment");
    EXPECT(check(mem, mem + k, &p, mem, 1, mem, 1, mem, &all, nullptr, &err), "grid_route: dist2 must be 4-byte aligned", "dist2 + k");
    EXPECT(check(mem, nullptr, &p, mem + k, 1, mem, 1, mem, &all, nullptr, &err), "grid_route: goals must be 4-byte aligned", "goals + k");
    EXPECT(check(mem, nullptr, &p, mem, 1, mem + k, 1, mem, &all, nullptr, &err), "grid_route: starts must be 4-byte aligned", "starts + k");
  }
  for (int k = 1; k < 8; ++k) {
    EXPECT(check(mem, nullptr, &p, mem, 1, mem, 1, mem + k, &all, nullptr, &err), "grid_route: workspace must be 8-byte aligned", "workspace + k");
    EXPECT(check(mem, nullptr, &p, mem, 1, mem, 1, mem, &all, mem + k, &err), "grid_route: counts must be 8-byte aligned", "counts + k");
  }
  // the outputs' alignment is named before the inputs', the workspace's before the counts'
  O q = all;
  q.cost = reinterpret_cast<uint32_t*>(mem + 2);
  EXPECT(check(mem, mem + 1, &p, mem + 1, 1, mem + 1, 1, mem + 1, &q, mem + 1, &err), "grid_route: cost must be 4-byte aligned", "every alignment off");
  EXPECT(check(mem, mem + 1, &p, mem + 1, 1, mem + 1, 1, mem + 1, &all, mem + 1, &err), "grid_route: dist2 must be 4-byte aligned", "the inputs and the rest off");
  EXPECT(check(mem, nullptr, &p, mem, 1, mem, 1, mem + 1, &all, mem + 1, &err), "grid_route: workspace must be 8-byte aligned", "workspace and counts off");
  EXPECT(route_out_check(nullptr, 0, false, &err), "grid_route: null out", "host: null out");
  EXPECT(route_out_check(&none, 0, false, &err), "grid_route: null cost", "host: null cost");
  // a refused parameter set is named before the lists and the workspace
  bad = good();
  bad.max_rounds = 0;
  EXPECT(check(mem, nullptr, &bad, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, &err), "grid_route: max_rounds outside 1..4096", "parameters before the lists");
}

static size_t up(size_t cells) { return (cells + T - 1) / T; }

static void sizes_and_defaults() {
  static_assert(T * T % ROUTE_THREADS == 0 && ROUTE_MAX_SWEEPS == 4 * T && ROUTE_HEADER_WORDS * 4 % 8 == 0, "the tile and the header");
  // tiles at 1 x 1, T - 1, T, T + 1, the largest grid and past 2^32
  CHECK(route_tiles_along(1) == 1 && route_tiles_along(T - 1) == 1 && route_tiles_along(T) == 1 && route_tiles_along(T + 1) == 2, "tiles along a side");
  CHECK(route_tiles_along(0) == 0 && route_tiles_along(-5) == 0 && route_tiles_along(INT_MIN) == 0, "tiles along nothing");
  CHECK(route_tiles_along(8192) == 8192u / T && route_tiles_along(INT_MAX) == up((size_t)INT_MAX), "tiles along the longest side and INT_MAX, no wrap");
  CHECK(route_tiles(1, 1) == 1 && route_tiles(T - 1, T - 1) == 1 && route_tiles(T, T) == 1 && route_tiles(T + 1, T + 1) == 4 && route_tiles(T + 1, T) == 2, "tiles");
  CHECK(route_tiles(2 * T + 1, T - 1) == 3 && route_tiles(130, 300) == up(130) * up(300), "tiles of the tests' shapes");
  CHECK(route_tiles(8192, 2048) == (size_t)(8192 / T) * (2048 / T) && route_tiles(8192, 2048) <= 65536, "the largest grid: %zu", route_tiles(8192, 2048));
  CHECK(route_tiles(8192, 1) == 8192u / T && route_tiles(8191, 2048) == up(8191) * (2048u / T), "thin and odd grids");
  CHECK(route_tiles(INT_MAX, INT_MAX) == up((size_t)INT_MAX) * up((size_t)INT_MAX) && route_tiles(INT_MAX, INT_MAX) > ((size_t)1 << 32), "past 2^32 tiles, in size_t");
  CHECK(route_groups(1) == 1 && route_groups(256) == 1 && route_groups(257) == 2 && route_groups((size_t)1 << 24) == 65536 && route_groups(0) == 0, "groups");
  CHECK(route_groups(65536) == 256 && route_groups(4096) == 16 && route_groups((size_t)5 << 32) == (size_t)5 << 24, "groups of the lists and past 2^32");
  // the workspace: header | two activity arrays | a byte per cell, rounded up to 8
  CHECK(route_ws_activity_offset(0, 7, 9) == 64 && route_ws_activity_offset(1, 7, 9) == 68 && route_ws_next_offset(7, 9) == 72, "layout of one tile");
  CHECK(route_workspace_bytes(1, 1) == 80 && route_workspace_bytes(7, 9) == 72 + 64 && route_workspace_bytes(1, 8) == 80 && route_workspace_bytes(1, 9) == 88, "workspace of one tile");
  CHECK(route_workspace_bytes(256, 256) == 64 + 8 * route_tiles(256, 256) + 65536, "workspace of a ground plan");
  CHECK(route_workspace_bytes(8192, 2048) == 64 + 8 * route_tiles(8192, 2048) + ((size_t)1 << 24), "the largest grid");
  CHECK(route_workspace_bytes(0, 5) == 0 && route_workspace_bytes(5, -1) == 0 && route_workspace_bytes(INT_MIN, INT_MIN) == 0, "workspace of nothing");
  CHECK(route_workspace_bytes(40000, 40000) == 64 + 8 * up(40000) * up(40000) + (size_t)1600000000ull, "past 2^32");
  CHECK(route_workspace_bytes(INT_MAX, INT_MAX) == ((64 + 8 * route_tiles(INT_MAX, INT_MAX) + (size_t)INT_MAX * (size_t)INT_MAX + 7) & ~(size_t)7), "INT_MAX squared, in size_t");
  for (int na : {1, T - 1, T, T + 1, 130})
    for (int nb : {1, T, T + 1, 300}) {
      CHECK(route_workspace_bytes(na, nb) % 8 == 0 && route_ws_next_offset(na, nb) + (size_t)na * nb <= route_workspace_bytes(na, nb), "%d x %d", na, nb);
      CHECK(route_ws_activity_offset(1, na, nb) - route_ws_activity_offset(0, na, nb) == 4 * route_tiles(na, nb), "%d x %d: the arrays do not overlap", na, nb);
    }
  svo_grid_clearance_params c{};
  c.na = 256; c.nb = 200; c.source_mask = 4; c.max_dist = 64; c.cell_size = 0.5; c.inflate_radius = 1.0;
  P p{};
  p.resume = 9; p.near_r2 = 9; p.near_weight = 9;
  CHECK(route_default_params(&c, &p) == SVO_OK, "defaults");
  CHECK(p.na == 256 && p.nb == 200 && p.near_r2 == 0 && p.near_weight == 0 && p.max_cost == 0x7F000000u && p.max_rounds == 64 && p.max_path == 4096 && p.resume == 0,
        "the defaults' values");
  const char* err = nullptr;
  CHECK(route_params_check(&p, 1, &err) == SVO_OK, "the defaults pass the check");
  CHECK(route_default_params(nullptr, &p) == SVO_ERR_INVALID && route_default_params(&c, nullptr) == SVO_ERR_INVALID, "null");
  for (int n : {0, 8193, INT_MIN}) {
    svo_grid_clearance_params h = c; h.na = n; CHECK(route_default_params(&h, &p) == SVO_ERR_INVALID, "na %d", n);
    h = c; h.nb = n; CHECK(route_default_params(&h, &p) == SVO_ERR_INVALID, "nb %d", n);
  }
  svo_grid_clearance_params h = c; h.na = 8192; h.nb = 2049;
  CHECK(route_default_params(&h, &p) == SVO_ERR_INVALID, "too many cells");
  h.nb = 2048;
  CHECK(route_default_params(&h, &p) == SVO_OK && p.na == 8192 && p.nb == 2048, "the largest grid's defaults");
  // one step stays below 2^23 and a candidate below 2^31 + 2^23 at the largest penalty and cap the checks let through
  CHECK(7ull * (16 + ROUTE_MAX_PENALTY) < (1ull << 23) && (unsigned long long)ROUTE_MAX_COST + 7ull * (16 + ROUTE_MAX_PENALTY) < (1ull << 32), "no wrap in u32");
}

int main() {
  params();
  pointers();
  sizes_and_defaults();
  if (fails) { fprintf(stderr, "%d failures\n", fails); return 1; }
  printf("grid route args ok\n");
  return 0;
}
