// The voxel map route's GPU-free logic (stereo_vo_amd/host/voxel_route.h) walked on the host, under ASan + UBSan: every refusal at
// its boundary with its code and its exact message and the accepted side of each boundary, the order of the refusals, the workspace's
// size and layout, the tile counts and the launch geometry at 64 x 1 x 1, at t - 1, t, t + 1 of each tile edge, at 2048 x 2048 x 256
// and in size_t past 2^32, the defaults, cell_of against the distance field's rule 9, and the header's per-cell statements relaxing a
// small volume to its fixed point, checked against a brute-force Bellman-Ford written here.
#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <initializer_list>
#include <vector>

#include "voxel_route.h"

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { ++fails; fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

// rc is the refusal with exactly this message, or (want == nullptr) SVO_OK with the message untouched
static void expect(int rc, const char* err, const char* want, const char* where) {
  if (want) CHECK(rc == SVO_ERR_INVALID && err && strcmp(err, want) == 0, "%s: rc %d, message '%s', wanted '%s'", where, rc, err ? err : "(none)", want);
  else CHECK(rc == SVO_OK && err == nullptr, "%s: rc %d, message '%s', wanted acceptance", where, rc, err ? err : "(none)");
}

// the check runs first: its message is read only after it returned
#define EXPECT(call, want, where) do { const char* err = nullptr; const int rc_ = (call); expect(rc_, err, want, where); } while (0)

using P = svo_voxel_route_params;
using O = svo_voxel_route_out;
constexpr int TX = VOXEL_ROUTE_TX, TY = VOXEL_ROUTE_TY, TZ = VOXEL_ROUTE_TZ;

static P good() {
  P p;
  p.near_r2 = 16; p.near_weight = 3; p.max_cost = 0x7F000000u; p.max_rounds = 64; p.max_path = 4096; p.resume = 0;
  return p;
}

template <typename F>
static void param_case(F change, const char* want, const char* where, int n_starts = 1) {
  P p = good();
  change(p);
  EXPECT(voxel_route_params_check(&p, n_starts, &err), want, where);
}

static void params() {
  const char *r2 = "voxel_route: near_r2 beyond 254^2", *pen = "voxel_route: near_weight * near_r2 beyond 2^20";
  const char *mc = "voxel_route: max_cost outside 1..0x7F000000", *mr = "voxel_route: max_rounds outside 1..4096";
  const char *mp = "voxel_route: max_path outside 1..2^20", *rs = "voxel_route: resume must be 0 or 1";
  EXPECT(voxel_route_params_check(nullptr, 0, &err), "voxel_route: null params", "null params");
  param_case([](P&) {}, nullptr, "a good set");
  param_case([](P& p) { p.near_r2 = 0; p.near_weight = 0xFFFFFFFFu; }, nullptr, "near_r2 0 under any weight");
  param_case([](P& p) { p.near_r2 = 254 * 254; p.near_weight = 0; }, nullptr, "near_r2 254^2");
  param_case([](P& p) { p.near_r2 = 254 * 254 + 1; p.near_weight = 0; }, r2, "near_r2 254^2 + 1");
  param_case([](P& p) { p.near_r2 = 0xFFFFu; p.near_weight = 0; }, r2, "near_r2 0xFFFF");
  param_case([](P& p) { p.near_r2 = 0xFFFFFFFFu; p.near_weight = 0; }, r2, "near_r2 all ones");
  param_case([](P& p) { p.near_r2 = 1u << 10; p.near_weight = 1u << 10; }, nullptr, "a penalty of 2^20");
  param_case([](P& p) { p.near_r2 = 1u << 10; p.near_weight = (1u << 10) + 1; }, pen, "a penalty of 2^20 + 2^10");
  param_case([](P& p) { p.near_r2 = 1; p.near_weight = 1u << 20; }, nullptr, "weight 2^20 at r2 1");
  param_case([](P& p) { p.near_r2 = 1; p.near_weight = (1u << 20) + 1; }, pen, "weight 2^20 + 1 at r2 1");
  param_case([](P& p) { p.near_r2 = 1u << 15; p.near_weight = 1u << 17; }, pen, "a product of 2^32: no 32-bit wrap to 0");
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
  param_case([](P& p) { p.near_r2 = 70000; p.max_cost = 0; p.resume = 7; }, r2, "several at once");
  param_case([](P& p) { p.max_cost = 0; p.max_rounds = 0; }, mc, "max_cost before max_rounds");
  param_case([](P& p) { p.max_path = 0; p.resume = 7; }, mp, "max_path before resume");
}

static void pointers() {
  alignas(8) static unsigned char mem[64];
  const P p = good();
  const int dims[3] = {128, 17, 9};
  O o{};
  o.cost = reinterpret_cast<uint32_t*>(mem);
  O all{reinterpret_cast<uint32_t*>(mem), mem + 1, reinterpret_cast<uint32_t*>(mem + 4), reinterpret_cast<uint32_t*>(mem + 8), mem + 13};
  auto check = [&](const void* closed, const int* d, const void* dist2, const P* prm, const void* goals, int ng, const void* starts, int ns, const void* ws,
                   const O* out, const void* counts, const char** err) { return voxel_route_check(closed, d, dist2, prm, goals, ng, starts, ns, ws, out, counts, err); };
  EXPECT(check(mem, dims, nullptr, &p, mem, 1, nullptr, 0, mem, &o, nullptr, &err), nullptr, "cost alone, no dist2, no starts, no counts");
  EXPECT(check(mem + 8, dims, mem + 2, &p, mem, 65536, mem + 8, 4096, mem + 8, &all, mem + 16, &err), nullptr, "everything, the largest lists");
  // the order: params, dims, closed, goals and starts, workspace, out and cost, the paths' consistency, the alignments
  EXPECT(check(nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, -1, nullptr, nullptr, nullptr, &err), "voxel_route: null params", "everything null: params first");
  P bad = good();
  bad.max_rounds = 0;
  EXPECT(check(nullptr, nullptr, nullptr, &bad, nullptr, 0, nullptr, -1, nullptr, nullptr, nullptr, &err), "voxel_route: max_rounds outside 1..4096", "the params' ranges before dims");
  EXPECT(check(nullptr, nullptr, nullptr, &p, nullptr, 0, nullptr, -1, nullptr, nullptr, nullptr, &err), "voxel_map_occupancy: null dims", "then dims");
  const int d_zero[3] = {64, 0, 1}, d_big[3] = {64, 2049, 1}, d_odd[3] = {96, 1, 1}, d_many[3] = {2048, 2048, 257}, d_most[3] = {2048, 2048, 256}, d_one[3] = {64, 1, 1};
  EXPECT(check(nullptr, d_zero, nullptr, &p, nullptr, 0, nullptr, -1, nullptr, nullptr, nullptr, &err), "voxel_map_occupancy: dims outside 1..2048", "a dimension of 0");
  EXPECT(check(nullptr, d_big, nullptr, &p, nullptr, 0, nullptr, -1, nullptr, nullptr, nullptr, &err), "voxel_map_occupancy: dims outside 1..2048", "a dimension of 2049");
  EXPECT(check(nullptr, d_odd, nullptr, &p, nullptr, 0, nullptr, -1, nullptr, nullptr, nullptr, &err), "voxel_map_occupancy: dims[0] must be a multiple of 64", "dims[0] 96");
  EXPECT(check(nullptr, d_many, nullptr, &p, nullptr, 0, nullptr, -1, nullptr, nullptr, nullptr, &err), "voxel_map_occupancy: dims[0] * dims[1] * dims[2] beyond 2^30", "2^30 + 2^22 cells");
  EXPECT(check(mem, d_most, nullptr, &p, mem, 1, nullptr, 0, mem, &o, nullptr, &err), nullptr, "2^30 cells");
  EXPECT(check(mem, d_one, nullptr, &p, mem, 1, nullptr, 0, mem, &o, nullptr, &err), nullptr, "64 x 1 x 1");
  EXPECT(check(nullptr, dims, nullptr, &p, nullptr, 0, nullptr, -1, nullptr, nullptr, nullptr, &err), "voxel_route: null closed", "then closed");
  for (int k = 1; k < 8; ++k) EXPECT(check(mem + k, dims, nullptr, &p, nullptr, 0, nullptr, -1, nullptr, nullptr, nullptr, &err), "voxel_route: closed must be 8-byte aligned", "closed + k");
  EXPECT(check(mem, dims, nullptr, &p, nullptr, 0, nullptr, -1, nullptr, nullptr, nullptr, &err), "voxel_route: null goals", "then goals");
  EXPECT(check(mem, dims, nullptr, &p, mem, 0, nullptr, -1, nullptr, nullptr, nullptr, &err), "voxel_route: n_goals outside 1..65536", "then n_goals");
  EXPECT(check(mem, dims, nullptr, &p, mem, 65537, nullptr, 0, mem, &o, nullptr, &err), "voxel_route: n_goals outside 1..65536", "n_goals 65537");
  EXPECT(check(mem, dims, nullptr, &p, mem, INT_MIN, nullptr, 0, mem, &o, nullptr, &err), "voxel_route: n_goals outside 1..65536", "n_goals INT_MIN");
  EXPECT(check(mem, dims, nullptr, &p, mem, 1, nullptr, -1, nullptr, nullptr, nullptr, &err), "voxel_route: n_starts outside 0..4096", "then n_starts");
  EXPECT(check(mem, dims, nullptr, &p, mem, 1, mem, 4097, mem, &all, nullptr, &err), "voxel_route: n_starts outside 0..4096", "n_starts 4097");
  EXPECT(check(mem, dims, nullptr, &p, mem, 1, nullptr, 1, nullptr, nullptr, nullptr, &err), "voxel_route: null starts with n_starts > 0", "then starts");
  EXPECT(check(mem, dims, nullptr, &p, mem, 1, mem, 0, nullptr, nullptr, nullptr, &err), "voxel_route: starts with n_starts == 0", "starts are NULL iff n_starts is 0");
  EXPECT(check(mem, dims, nullptr, &p, mem, 1, mem, 1, nullptr, nullptr, nullptr, &err), "voxel_route: null workspace", "then the workspace");
  EXPECT(check(mem, dims, nullptr, &p, mem, 1, mem, 1, mem, nullptr, nullptr, &err), "voxel_route: null out", "then out");
  O none{};
  EXPECT(check(mem, dims, nullptr, &p, mem, 1, mem, 1, mem, &none, nullptr, &err), "voxel_route: null cost", "then cost");
  const char* together = "voxel_route: path, path_len and path_status go together";
  for (int miss = 1; miss < 7; ++miss) {  // every proper, non-empty subset of the three left out
    O q = all;
    if (miss & 1) q.path = nullptr;
    if (miss & 2) q.path_len = nullptr;
    if (miss & 4) q.path_status = nullptr;
    EXPECT(check(mem, dims, nullptr, &p, mem, 1, mem, 1, mem, &q, nullptr, &err), together, "a part of the path outputs");
    EXPECT(voxel_route_out_check(&q, 1, &err), together, "host: a part of the path outputs");
  }
  EXPECT(check(mem, dims, nullptr, &p, mem, 1, nullptr, 0, mem, &all, nullptr, &err), "voxel_route: path outputs with n_starts == 0", "path outputs without starts");
  EXPECT(check(mem, dims, nullptr, &p, mem, 1, mem, 3, mem, &o, nullptr, &err), nullptr, "starts without path outputs");
  bad = good();
  bad.max_path = 0;
  EXPECT(check(mem, dims, nullptr, &bad, mem, 1, mem, 1, mem, &all, nullptr, &err), "voxel_route: max_path outside 1..2^20", "max_path with starts");
  EXPECT(check(mem, dims, nullptr, &bad, mem, 1, nullptr, 0, mem, &o, nullptr, &err), nullptr, "max_path is not read without starts");
  for (int k = 1; k < 4; ++k) {
    O q = all;
    q.cost = reinterpret_cast<uint32_t*>(mem + k);
    EXPECT(check(mem, dims, nullptr, &p, mem, 1, mem, 1, mem, &q, nullptr, &err), "voxel_route: cost must be 4-byte aligned", "cost + k");
    EXPECT(voxel_route_out_check(&q, 1, &err), nullptr, "host cost of any alignment");
    q = all;
    q.path = reinterpret_cast<uint32_t*>(mem + k);
    EXPECT(check(mem, dims, nullptr, &p, mem, 1, mem, 1, mem, &q, nullptr, &err), "voxel_route: path must be 4-byte aligned", "path + k");
    q = all;
    q.path_len = reinterpret_cast<uint32_t*>(mem + k);
    EXPECT(check(mem, dims, nullptr, &p, mem, 1, mem, 1, mem, &q, nullptr, &err), "voxel_route: path_len must be 4-byte aligned", "path_len + k");
    q = all;
    q.next = mem + k; q.path_status = mem + k;
    EXPECT(check(mem, dims, nullptr, &p, mem, 1, mem, 1, mem, &q, nullptr, &err), nullptr, "next and path_status of any alignment");
    EXPECT(check(mem, dims, nullptr, &p, mem + k, 1, mem, 1, mem, &all, nullptr, &err), "voxel_route: goals must be 4-byte aligned", "goals + k");
    EXPECT(check(mem, dims, nullptr, &p, mem, 1, mem + k, 1, mem, &all, nullptr, &err), "voxel_route: starts must be 4-byte aligned", "starts + k");
  }
  EXPECT(check(mem, dims, mem + 1, &p, mem, 1, mem, 1, mem, &all, nullptr, &err), "voxel_route: dist2 must be 2-byte aligned", "dist2 + 1");
  EXPECT(check(mem, dims, mem + 2, &p, mem, 1, mem, 1, mem, &all, nullptr, &err), nullptr, "dist2 + 2");
  for (int k = 1; k < 8; ++k) {
    EXPECT(check(mem, dims, nullptr, &p, mem, 1, mem, 1, mem + k, &all, nullptr, &err), "voxel_route: workspace must be 8-byte aligned", "workspace + k");
    EXPECT(check(mem, dims, nullptr, &p, mem, 1, mem, 1, mem, &all, mem + k, &err), "voxel_route: counts must be 8-byte aligned", "counts + k");
  }
  // among the alignments: cost, goals, starts, path, path_len, dist2, workspace, counts
  O q = all;
  q.cost = reinterpret_cast<uint32_t*>(mem + 2);
  EXPECT(check(mem, dims, mem + 1, &p, mem + 1, 1, mem + 1, 1, mem + 1, &q, mem + 1, &err), "voxel_route: cost must be 4-byte aligned", "every alignment off");
  EXPECT(check(mem, dims, mem + 1, &p, mem + 1, 1, mem + 1, 1, mem + 1, &all, mem + 1, &err), "voxel_route: goals must be 4-byte aligned", "the inputs and the rest off");
  EXPECT(check(mem, dims, mem + 1, &p, mem, 1, mem, 1, mem + 1, &all, mem + 1, &err), "voxel_route: dist2 must be 2-byte aligned", "dist2, workspace and counts off");
  EXPECT(check(mem, dims, nullptr, &p, mem, 1, mem, 1, mem + 1, &all, mem + 1, &err), "voxel_route: workspace must be 8-byte aligned", "workspace and counts off");
  // the paths' consistency is named before any alignment
  q = all;
  q.path = nullptr; q.cost = reinterpret_cast<uint32_t*>(mem + 2);
  EXPECT(check(mem, dims, nullptr, &p, mem, 1, mem, 1, mem, &q, nullptr, &err), together, "consistency before alignment");
  // the host form: resume refused after the ranges, no workspace, host arrays of any alignment
  auto host = [&](const void* closed, const int* d, const void* dist2, const P* prm, const void* goals, int ng, const void* starts, int ns, const O* out, const char** err) {
    return voxel_route_host_check(closed, d, dist2, prm, goals, ng, starts, ns, out, err);
  };
  q = all;
  q.cost = reinterpret_cast<uint32_t*>(mem + 1); q.path = reinterpret_cast<uint32_t*>(mem + 3); q.path_len = reinterpret_cast<uint32_t*>(mem + 5);
  EXPECT(host(mem, dims, mem + 2, &p, mem + 1, 1, mem + 3, 1, &q, &err), nullptr, "host arrays of any alignment");
  bad = good();
  bad.resume = 1;
  EXPECT(host(nullptr, nullptr, nullptr, &bad, nullptr, 0, nullptr, 0, nullptr, &err), "voxel_route: resume needs the _dev entry, whose workspace outlives the call", "host: resume");
  bad.max_cost = 0;
  EXPECT(host(nullptr, nullptr, nullptr, &bad, nullptr, 0, nullptr, 0, nullptr, &err), "voxel_route: max_cost outside 1..0x7F000000", "host: the ranges before resume");
  EXPECT(host(nullptr, nullptr, nullptr, &p, nullptr, 0, nullptr, 0, nullptr, &err), "voxel_map_occupancy: null dims", "host: dims");
  EXPECT(host(nullptr, dims, nullptr, &p, nullptr, 0, nullptr, 0, nullptr, &err), "voxel_route: null closed", "host: closed");
  EXPECT(host(mem + 4, dims, nullptr, &p, nullptr, 0, nullptr, 0, nullptr, &err), "voxel_route: closed must be 8-byte aligned", "host: closed stays a device pointer");
  EXPECT(host(mem, dims, nullptr, &p, nullptr, 0, nullptr, 0, nullptr, &err), "voxel_route: null goals", "host: goals");
  EXPECT(host(mem, dims, nullptr, &p, mem, 1, nullptr, 0, nullptr, &err), "voxel_route: null out", "host: out");
  EXPECT(host(mem, dims, nullptr, &p, mem, 1, nullptr, 0, &none, &err), "voxel_route: null cost", "host: cost");
  EXPECT(host(mem, dims, nullptr, &p, mem, 1, nullptr, 0, &all, &err), "voxel_route: path outputs with n_starts == 0", "host: path outputs without starts");
  EXPECT(host(mem, dims, mem + 1, &p, mem, 1, nullptr, 0, &o, &err), "voxel_route: dist2 must be 2-byte aligned", "host: dist2 stays a device pointer");
}

static size_t up(size_t cells, size_t t) { return (cells + t - 1) / t; }

static void sizes_and_defaults() {
  static_assert(TX * TY * TZ % VOXEL_ROUTE_THREADS == 0 && VOXEL_ROUTE_HEADER_WORDS * 4 % 8 == 0 && VOXEL_ROUTE_MAX_SWEEPS >= TX + TY + TZ, "the tile and the header");
  static_assert((TX + 2) * (TY + 2) * (TZ + 2) * 13 <= 64 * 1024, "a tile with its halo fits the LDS of a workgroup: 13 bytes per cell");
  for (int t : {TX, TY, TZ}) {
    CHECK(voxel_route_tiles_along(1, t) == 1 && voxel_route_tiles_along(t - 1, t) == (t > 1 ? 1u : 0u) && voxel_route_tiles_along(t, t) == 1 && voxel_route_tiles_along(t + 1, t) == 2,
          "tiles along an axis, edge %d", t);
    CHECK(voxel_route_tiles_along(0, t) == 0 && voxel_route_tiles_along(-5, t) == 0 && voxel_route_tiles_along(INT_MIN, t) == 0, "tiles along nothing");
    CHECK(voxel_route_tiles_along(2048, t) == 2048u / t && voxel_route_tiles_along(INT_MAX, t) == up((size_t)INT_MAX, t), "the longest axis and INT_MAX, no wrap");
  }
  auto tiles = [](int a, int b, int c) { const int d[3] = {a, b, c}; return voxel_route_tiles(d); };
  CHECK(tiles(64, 1, 1).total == 64u / TX && tiles(64, 1, 1).n0 == 64u / TX && tiles(64, 1, 1).n1 == 1 && tiles(64, 1, 1).n2 == 1, "64 x 1 x 1");
  // t - 1, t, t + 1 of each edge (the tile functions take any dims; the entry's dims[0] is a multiple of 64)
  CHECK(tiles(TX - 1, TY - 1, TZ - 1).total == 1 && tiles(TX, TY, TZ).total == 1 && tiles(TX + 1, TY, TZ).total == 2 && tiles(TX, TY + 1, TZ).total == 2 &&
        tiles(TX, TY, TZ + 1).total == 2 && tiles(TX + 1, TY + 1, TZ + 1).total == 8, "one tile and its neighbours");
  CHECK(tiles(64, TY - 1, TZ + 1).total == (64u / TX) * 2 && tiles(128, 33, 17).total == up(128, TX) * up(33, TY) * up(17, TZ), "the tests' shapes");
  CHECK(tiles(2048, 2048, 256).total == (size_t)(2048 / TX) * (2048 / TY) * (256 / TZ) && tiles(2048, 2048, 256).total == ((size_t)1 << 30) / (TX * TY * TZ), "the largest volume");
  CHECK(tiles(512, 128, 512).total == ((size_t)1 << 25) / (TX * TY * TZ), "the default volume: %zu", tiles(512, 128, 512).total);
  CHECK(tiles(INT_MAX, INT_MAX, 1).total == up((size_t)INT_MAX, TX) * up((size_t)INT_MAX, TY) && tiles(INT_MAX, INT_MAX, 1).total > ((size_t)1 << 32), "past 2^32 tiles, in size_t");
  CHECK(voxel_route_groups(1) == 1 && voxel_route_groups(256) == 1 && voxel_route_groups(257) == 2 && voxel_route_groups((size_t)1 << 30) == (size_t)1 << 22 && voxel_route_groups(0) == 0,
        "groups");
  CHECK(voxel_route_groups(65536) == 256 && voxel_route_groups(4096) == 16 && voxel_route_groups((size_t)5 << 32) == (size_t)5 << 24, "groups of the lists and past 2^32");
  // the workspace: header | two activity arrays | a byte per cell, rounded up to 8
  const int d1[3] = {64, 1, 1}, d2[3] = {128, 33, 17}, d3[3] = {2048, 2048, 256}, d4[3] = {64, 3, 3};
  size_t b = 1;
  CHECK(voxel_route_ws_activity_offset(0, d1) == 64 && voxel_route_ws_activity_offset(1, d1) == 64 + 4 * (64u / TX) && voxel_route_ws_next_offset(d1) == 64 + 8 * (64u / TX), "layout of 64 x 1 x 1");
  CHECK(voxel_route_workspace_bytes(d1, &b) == SVO_OK && b == 64 + 8 * (64u / TX) + 64, "workspace of 64 x 1 x 1: %zu", b);
  CHECK(voxel_route_workspace_bytes(d2, &b) == SVO_OK && b == 64 + 8 * tiles(128, 33, 17).total + 128 * 33 * 17, "workspace of 128 x 33 x 17: %zu", b);
  CHECK(voxel_route_workspace_bytes(d3, &b) == SVO_OK && b == 64 + 8 * tiles(2048, 2048, 256).total + ((size_t)1 << 30) && b > ((size_t)1 << 30), "the largest volume: %zu", b);
  CHECK(voxel_route_workspace_bytes(d4, &b) == SVO_OK && b % 8 == 0 && b >= voxel_route_ws_next_offset(d4) + 64 * 9, "64 x 3 x 3: %zu", b);
  for (const int* d : {d1, d2, d3, d4})
    CHECK(voxel_route_ws_activity_offset(1, d) - voxel_route_ws_activity_offset(0, d) == 4 * voxel_route_tiles(d).total && voxel_route_ws_next_offset(d) % 8 == 0, "the arrays do not overlap");
  const int bad1[3] = {96, 1, 1}, bad2[3] = {64, 0, 1}, bad3[3] = {2048, 2048, 257};
  for (const int* d : {bad1, bad2, bad3}) {
    b = 5;
    CHECK(voxel_route_workspace_bytes(d, &b) == SVO_ERR_INVALID && b == 0, "refused dims");
  }
  b = 5;
  CHECK(voxel_route_workspace_bytes(nullptr, &b) == SVO_ERR_INVALID && b == 0 && voxel_route_workspace_bytes(d1, nullptr) == SVO_ERR_INVALID, "null");
  P p{};
  p.resume = 9; p.near_r2 = 9; p.near_weight = 9;
  CHECK(voxel_route_default_params(0.1f, &p) == SVO_OK, "defaults");
  CHECK(p.near_r2 == 0 && p.near_weight == 0 && p.max_cost == 0x7F000000u && p.max_rounds == 32 && p.max_path == 4096 && p.resume == 0, "the defaults' values");
  const char* err = nullptr;
  CHECK(voxel_route_params_check(&p, 1, &err) == SVO_OK, "the defaults pass the check");
  CHECK(voxel_route_default_params(0.1f, nullptr) == SVO_ERR_INVALID && voxel_route_default_params(0.0f, &p) == SVO_ERR_INVALID && voxel_route_default_params(-1.0f, &p) == SVO_ERR_INVALID &&
        voxel_route_default_params(NAN, &p) == SVO_ERR_INVALID && voxel_route_default_params(INFINITY, &p) == SVO_ERR_INVALID, "refused defaults");
  // one step stays below 2^24 and a candidate below 2^32 at the largest penalty and cap the checks let through
  CHECK(9ull * (16 + VOXEL_ROUTE_MAX_PENALTY) < (1ull << 24) && (unsigned long long)VOXEL_ROUTE_MAX_COST + 9ull * (16 + VOXEL_ROUTE_MAX_PENALTY) < (1ull << 32), "no wrap in u32");
  CHECK(VOXEL_ROUTE_MAX_NEAR_R2 < VOXEL_DISTANCE_NONE16, "NONE16 is below no near_r2");
}

// rule 9 of the distance field, restated: q = x / voxel_size in doubles from the widened floats, j = floor(q) - origin
static void cell_of() {
  const int origin[3] = {-61, -3, -7}, dims[3] = {128, 9, 13};
  const float vs = 0.25f;
  int inside = 0, outside = 0;
  for (int i = -70; i <= 70; ++i)
    for (int j = -5; j <= 7; ++j) {
      const float xyz[3] = {(float)(0.249 * i + 0.01), (float)(0.26 * j - 0.02), (float)(0.37 * j + 0.11)};
      long long q[3];
      bool in = true;
      for (int r = 0; r < 3; ++r) {
        q[r] = (long long)floor((double)xyz[r] / (double)vs) - origin[r];
        in = in && q[r] >= 0 && q[r] < dims[r];
      }
      uint32_t cell = 77;
      const int rc = voxel_occupancy_cell_of(vs, origin, dims, xyz, &cell);
      if (in) { ++inside; CHECK(rc == SVO_OK && cell == (uint32_t)(q[0] + dims[0] * (q[1] + dims[1] * q[2])), "cell of (%g, %g, %g): %u", xyz[0], xyz[1], xyz[2], cell); }
      else { ++outside; CHECK(rc == SVO_ERR_INVALID && cell == 77, "outside (%g, %g, %g)", xyz[0], xyz[1], xyz[2]); }
    }
  CHECK(inside > 300 && outside > 300, "both kinds: %d inside, %d outside", inside, outside);
  uint32_t cell = 0;
  const float zero[3] = {0, 0, 0}, nan3[3] = {NAN, 0, 0}, inf3[3] = {0, INFINITY, 0}, far3[3] = {0, 0, 262140.0f}, edge[3] = {-15.25f, -0.75f, -1.75f};
  CHECK(voxel_occupancy_cell_of(vs, origin, dims, zero, &cell) == SVO_OK && cell == 61 + 128 * (3 + 9 * 7), "the origin of the world: %u", cell);
  CHECK(voxel_occupancy_cell_of(vs, origin, dims, edge, &cell) == SVO_OK && cell == 0, "the volume's first cell: %u", cell);
  CHECK(voxel_occupancy_cell_of(vs, origin, dims, nan3, &cell) == SVO_ERR_INVALID && voxel_occupancy_cell_of(vs, origin, dims, inf3, &cell) == SVO_ERR_INVALID &&
        voxel_occupancy_cell_of(vs, origin, dims, far3, &cell) == SVO_ERR_INVALID, "rejected positions");
  const int o_bad[3] = {1 << 20, 0, 0}, d_bad[3] = {100, 9, 13};
  CHECK(voxel_occupancy_cell_of(0.0f, origin, dims, zero, &cell) == SVO_ERR_INVALID && voxel_occupancy_cell_of(vs, o_bad, dims, zero, &cell) == SVO_ERR_INVALID &&
        voxel_occupancy_cell_of(vs, origin, d_bad, zero, &cell) == SVO_ERR_INVALID && voxel_occupancy_cell_of(vs, nullptr, dims, zero, &cell) == SVO_ERR_INVALID &&
        voxel_occupancy_cell_of(vs, origin, nullptr, zero, &cell) == SVO_ERR_INVALID && voxel_occupancy_cell_of(vs, origin, dims, nullptr, &cell) == SVO_ERR_INVALID &&
        voxel_occupancy_cell_of(vs, origin, dims, zero, nullptr) == SVO_ERR_INVALID, "refused arguments");
}

// ----------------------------------------------------------------------------- the per-cell statements against a brute force
static void codes() {
  int seen = 0;
  for (int c = -1; c <= 1; ++c)
    for (int b = -1; b <= 1; ++b)
      for (int a = -1; a <= 1; ++a) {
        const int k = voxel_route_code(a, b, c);
        CHECK(k == seen && voxel_route_d0(k) == a && voxel_route_d1(k) == b && voxel_route_d2(k) == c, "code %d", k);
        const int changed = (a != 0) + (b != 0) + (c != 0);
        if (k != VOXEL_ROUTE_SELF) CHECK(voxel_route_weight(k) == (changed == 1 ? 5u : changed == 2 ? 7u : 9u), "weight of %d", k);
        ++seen;
      }
  CHECK(seen == 27 && voxel_route_code(0, 0, 0) == VOXEL_ROUTE_SELF, "27 codes");
  // everything open allows all 26; the cell itself closed allows none; one face cell closed takes 9 moves with it, one edge cell 3 (itself and two vertex moves), one vertex cell 1
  const uint32_t all = (1u << 27) - 1;
  CHECK(voxel_route_allowed(all) == (all & ~(1u << VOXEL_ROUTE_SELF)) && voxel_route_allowed(all & ~(1u << VOXEL_ROUTE_SELF)) == 0 && voxel_route_allowed(0) == 0, "all and none");
  CHECK(__builtin_popcount(voxel_route_allowed(all & ~(1u << voxel_route_code(1, 0, 0)))) == 26 - 9, "a face cell closed");
  CHECK(__builtin_popcount(voxel_route_allowed(all & ~(1u << voxel_route_code(1, -1, 0)))) == 26 - 3, "an edge cell closed");
  CHECK(__builtin_popcount(voxel_route_allowed(all & ~(1u << voxel_route_code(-1, 1, 1)))) == 26 - 1, "a vertex cell closed");
  // the faces of a tile: the interior touches none, a corner seven neighbours, an edge cell three, a face cell one
  CHECK(voxel_route_faces(1, 1, 1, 8, 8, 8) == 0 && __builtin_popcount(voxel_route_faces(0, 0, 0, 8, 8, 8)) == 7 && __builtin_popcount(voxel_route_faces(7, 3, 0, 8, 8, 8)) == 3 &&
        voxel_route_faces(3, 7, 3, 8, 8, 8) == 1u << voxel_route_code(0, 1, 0), "faces of a cube");
  for (int l0 = 0; l0 < TX; ++l0)
    for (int l1 = 0; l1 < TY; ++l1)
      for (int l2 = 0; l2 < TZ; ++l2) {
        uint32_t want = 0;
        for (int k = 0; k < 27; ++k) {  // the neighbour tile's halo: its interior grown by one cell, in this tile's coordinates
          if (k == VOXEL_ROUTE_SELF) continue;
          const int o0 = voxel_route_d0(k) * TX, o1 = voxel_route_d1(k) * TY, o2 = voxel_route_d2(k) * TZ;
          if (l0 >= o0 - 1 && l0 <= o0 + TX && l1 >= o1 - 1 && l1 <= o1 + TY && l2 >= o2 - 1 && l2 <= o2 + TZ) want |= 1u << k;
        }
        CHECK(voxel_route_faces(l0, l1, l2, TX, TY, TZ) == want, "faces at (%d, %d, %d)", l0, l1, l2);
      }
}

struct Volume {
  int d0, d1, d2;
  std::vector<uint64_t> words;
  std::vector<uint16_t> dist2;
  bool closed(int j0, int j1, int j2) const {
    if (j0 < 0 || j0 >= d0 || j1 < 0 || j1 >= d1 || j2 < 0 || j2 >= d2) return true;
    const size_t B = (size_t)j0 + (size_t)d0 * ((size_t)j1 + (size_t)d1 * (size_t)j2);
    return (words[B >> 6] >> (B & 63)) & 1u;
  }
};

static void relax_to_the_fixed_point(int d0, int d1, int d2, unsigned seed, bool with_dist2, uint32_t max_cost, size_t min_reached) {
  Volume v{d0, d1, d2, {}, {}};
  const size_t n = (size_t)d0 * d1 * d2;
  v.words.assign(n / 64, 0);
  v.dist2.assign(n, 0);
  uint64_t s = seed * 0x9E3779B97F4A7C15ull + 1;
  auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
  for (size_t B = 0; B < n; ++B) {
    if (rnd() % 100 < 25) v.words[B >> 6] |= 1ull << (B & 63);
    v.dist2[B] = rnd() % 5 == 0 ? VOXEL_DISTANCE_NONE16 : (uint16_t)(rnd() % 41);
  }
  v.words[0] &= ~1ull;  // the goal
  VoxelRouteVolume g{v.words.data(), with_dist2 ? v.dist2.data() : nullptr, d0, d1, d2, 16u, 3u, max_cost};
  auto at = [&](int j0, int j1, int j2) { return (size_t)j0 + (size_t)d0 * ((size_t)j1 + (size_t)d1 * (size_t)j2); };
  // (a) the header's statements, cell by cell in place until a pass changes nothing
  std::vector<uint32_t> cost(n, VOXEL_ROUTE_NONE);
  cost[0] = 0;
  for (int pass = 0, changed = 1; changed; ++pass) {
    changed = 0;
    CHECK(pass <= (int)n, "the relaxation ends");
    if (pass > (int)n) break;
    for (int j2 = 0; j2 < d2; ++j2)
      for (int j1 = 0; j1 < d1; ++j1)
        for (int j0 = 0; j0 < d0; ++j0) {
          const size_t B = at(j0, j1, j2);
          const uint32_t allowed = voxel_route_allowed(voxel_route_open27(g, j0, j1, j2));
          auto nb = [&](int k) { return at(j0 + voxel_route_d0(k), j1 + voxel_route_d1(k), j2 + voxel_route_d2(k)); };
          const uint32_t b = voxel_route_relax(
              cost[B], allowed, max_cost, [&](int k) { return (allowed >> k) & 1u ? cost[nb(k)] : VOXEL_ROUTE_NONE; },
              [&](int k) { return (allowed >> k) & 1u ? voxel_route_weight(k) * voxel_route_unit(g, nb(k)) : 0u; });
          if (b != cost[B]) { cost[B] = b; changed = 1; }
        }
  }
  // (b) a brute force written here: whole sweeps over a copy, rule 2's box spelt out, in 64-bit sums
  std::vector<unsigned long long> want(n, ~0ull), prev;
  want[0] = 0;
  do {
    prev = want;
    for (int j2 = 0; j2 < d2; ++j2)
      for (int j1 = 0; j1 < d1; ++j1)
        for (int j0 = 0; j0 < d0; ++j0) {
          if (v.closed(j0, j1, j2)) continue;
          for (int c = -1; c <= 1; ++c)
            for (int b = -1; b <= 1; ++b)
              for (int a = -1; a <= 1; ++a) {
                if (!a && !b && !c) continue;
                bool open = true;
                for (int z = 0; z <= 1; ++z)
                  for (int y = 0; y <= 1; ++y)
                    for (int x = 0; x <= 1; ++x) open = open && !v.closed(j0 + x * a, j1 + y * b, j2 + z * c);
                if (!open) continue;
                const size_t u = at(j0 + a, j1 + b, j2 + c);
                if (prev[u] == ~0ull) continue;
                const int changed = (a != 0) + (b != 0) + (c != 0);
                unsigned long long pen = 0;
                if (with_dist2 && v.dist2[u] != 0xFFFF && v.dist2[u] < 16) pen = 3ull * (16 - v.dist2[u]);
                const unsigned long long cand = prev[u] + (unsigned long long)(3 + 2 * changed) * (16 + pen);
                if (cand <= max_cost && cand < want[at(j0, j1, j2)]) want[at(j0, j1, j2)] = cand;
              }
        }
  } while (prev != want);
  size_t reached = 0, differ = 0, next_bad = 0;
  for (size_t B = 0; B < n; ++B) {
    reached += want[B] != ~0ull;
    differ += (want[B] == ~0ull ? VOXEL_ROUTE_NONE : (uint32_t)want[B]) != cost[B];
  }
  CHECK(differ == 0 && reached >= min_reached, "%d x %d x %d seed %u: %zu cells differ, %zu reached", d0, d1, d2, seed, differ, reached);
  printf("%d x %d x %d seed %u: %zu of %zu cells reached\n", d0, d1, d2, seed, reached, n);
  // rule 5 and a step along it: following next from any reached cell lowers the cost and ends at the goal
  for (size_t B = 0; B < n; ++B) {
    const uint8_t k = voxel_route_next_one(g, cost.data(), B);
    if (cost[B] == VOXEL_ROUTE_NONE) { next_bad += k != VOXEL_ROUTE_NO_MOVE; continue; }
    if (cost[B] == 0) { next_bad += k != VOXEL_ROUTE_SELF || voxel_route_step((uint32_t)B, k, d0, d1, d2) != VOXEL_ROUTE_NONE; continue; }
    const uint32_t u = voxel_route_step((uint32_t)B, k, d0, d1, d2);
    if (k >= 27 || u == VOXEL_ROUTE_NONE || cost[u] >= cost[B]) { ++next_bad; continue; }
    for (int smaller = 0; smaller < k; ++smaller) {  // no smaller allowed k attains the cost
      const uint32_t allowed = voxel_route_allowed(voxel_route_open27(g, (int)(B % d0), (int)(B / d0 % d1), (int)(B / d0 / d1)));
      if (smaller == VOXEL_ROUTE_SELF || !((allowed >> smaller) & 1u)) continue;
      const uint32_t w = voxel_route_step((uint32_t)B, (unsigned)smaller, d0, d1, d2);
      next_bad += cost[w] != VOXEL_ROUTE_NONE && cost[w] + voxel_route_weight(smaller) * voxel_route_unit(g, w) == cost[B];
    }
  }
  CHECK(next_bad == 0, "%d x %d x %d seed %u: %zu directions are wrong", d0, d1, d2, seed, next_bad);
  CHECK(voxel_route_step(0, 12, d0, d1, d2) == VOXEL_ROUTE_NONE && voxel_route_step((uint32_t)d0 - 1, 14, d0, d1, d2) == VOXEL_ROUTE_NONE &&
        voxel_route_step(0, 255, d0, d1, d2) == VOXEL_ROUTE_NONE && voxel_route_step(0, 27, d0, d1, d2) == VOXEL_ROUTE_NONE, "a step that leaves the volume or is none");
  CHECK(d1 < 2 || voxel_route_step((uint32_t)d0 - 1, 17, d0, d1, d2) == VOXEL_ROUTE_NONE, "axis 0 does not run on into the next row");
}

int main() {
  params();
  pointers();
  sizes_and_defaults();
  cell_of();
  codes();
  relax_to_the_fixed_point(64, 5, 4, 1, false, VOXEL_ROUTE_MAX_COST, 900);
  relax_to_the_fixed_point(64, 5, 4, 2, true, VOXEL_ROUTE_MAX_COST, 900);
  relax_to_the_fixed_point(64, 3, 7, 3, true, 2500, 300);
  relax_to_the_fixed_point(128, 9, 1, 4, true, VOXEL_ROUTE_MAX_COST, 300);
  relax_to_the_fixed_point(64, 1, 1, 5, false, VOXEL_ROUTE_MAX_COST, 2);
  if (fails) { fprintf(stderr, "%d failures\n", fails); return 1; }
  printf("voxel route args ok\n");
  return 0;
}
