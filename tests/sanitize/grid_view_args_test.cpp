// The ground plan view's GPU-free host logic (stereo_vo_amd/host/view_args.h) walked on the host, under ASan + UBSan: every refusal at
// its boundary with its code and its exact message and the accepted side of each boundary, the order of the refusals, the workspace's
// size and layout, the window's words and LDS bytes, the ring enumeration (every offset of the square visited exactly once, ring by
// ring, for max_range 1, 2, 31, 32 and 255), the score at its edges, the defaults.
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "view_args.h"

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { ++fails; fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

// rc is the refusal with exactly this message, or (want == nullptr) SVO_OK with the message untouched
static void expect(int rc, const char* err, const char* want, const char* where) {
  if (want) CHECK(rc == SVO_ERR_INVALID && err && strcmp(err, want) == 0, "%s: rc %d, message '%s', wanted '%s'", where, rc, err ? err : "(none)", want);
  else CHECK(rc == SVO_OK && err == nullptr, "%s: rc %d, message '%s', wanted acceptance", where, rc, err ? err : "(none)");
}

// the check runs first: its message is read only after it returned
#define EXPECT(call, want, where) do { const char* err = nullptr; const int rc_ = (call); expect(rc_, err, want, where); } while (0)

using P = svo_grid_view_params;
using O = svo_grid_view_out;

static P good() {
  P p;
  p.na = 32; p.nb = 13; p.opaque_mask = 4u; p.gain_mask = 1u; p.max_range = 64; p.gain_weight = 16; p.cost_div = 1;
  return p;
}

alignas(16) static unsigned char mem[512];
static O full() {
  O o;
  o.records = reinterpret_cast<svo_grid_view_rec*>(mem + 16); o.order = reinterpret_cast<uint32_t*>(mem + 64);
  o.best = reinterpret_cast<uint32_t*>(mem + 128); o.seen = reinterpret_cast<uint32_t*>(mem + 192);
  return o;
}

template <typename F>
static void param_case(F change, const char* want, const char* where) {
  P p = good();
  change(p);
  EXPECT(view_params_check(&p, &err), want, where);
  const O o = full();
  EXPECT(view_check(mem, mem + 4, 8, mem + 4, &p, mem + 8, &o, mem + 8, true, &err), want, where);
  EXPECT(view_check(mem, mem + 1, 8, mem + 1, &p, nullptr, &o, mem + 1, false, &err), want, where);
  CHECK((view_workspace_bytes(p.na, p.nb, 8) == 0) == (p.na < 1 || p.na > 8192 || p.nb < 1 || p.nb > 8192 || (long long)p.na * p.nb > (1ll << 24)),
        "%s: the workspace is 0 exactly for a refused shape", where);
}

static void params() {
  const char *na = "grid_view: na outside 1..8192", *nb = "grid_view: nb outside 1..8192", *area = "grid_view: na * nb beyond 2^24";
  const char *om = "grid_view: opaque_mask is 0", *gm = "grid_view: gain_mask is 0", *mr = "grid_view: max_range outside 1..255";
  const char *gw = "grid_view: gain_weight outside 1..65536", *cd = "grid_view: cost_div outside 1..2^31";
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
  param_case([](P& p) { p.na = 8192; p.nb = 8192; }, area, "2^26 cells");
  param_case([](P& p) { p.opaque_mask = 0; }, om, "opaque_mask 0");
  param_case([](P& p) { p.opaque_mask = 0x80000000u; }, nullptr, "opaque_mask bit 31");
  param_case([](P& p) { p.gain_mask = 0; }, gm, "gain_mask 0");
  param_case([](P& p) { p.gain_mask = 0xFFFFFFFFu; p.opaque_mask = 0xFFFFFFFFu; }, nullptr, "every class both");
  param_case([](P& p) { p.opaque_mask = 5u; }, nullptr, "the masks share bit 0");
  param_case([](P& p) { p.max_range = 0; }, mr, "max_range 0");
  param_case([](P& p) { p.max_range = 1; }, nullptr, "max_range 1");
  param_case([](P& p) { p.max_range = 255; }, nullptr, "max_range 255");
  param_case([](P& p) { p.max_range = 256; }, mr, "max_range 256");
  param_case([](P& p) { p.max_range = -1; }, mr, "max_range -1");
  param_case([](P& p) { p.max_range = INT_MAX; }, mr, "max_range INT_MAX");
  param_case([](P& p) { p.gain_weight = 0; }, gw, "gain_weight 0");
  param_case([](P& p) { p.gain_weight = 1; }, nullptr, "gain_weight 1");
  param_case([](P& p) { p.gain_weight = 65536; }, nullptr, "gain_weight 65536");
  param_case([](P& p) { p.gain_weight = 65537; }, gw, "gain_weight 65537");
  param_case([](P& p) { p.gain_weight = 0xFFFFFFFFu; }, gw, "gain_weight 2^32 - 1");
  param_case([](P& p) { p.cost_div = 0; }, cd, "cost_div 0");
  param_case([](P& p) { p.cost_div = 1u << 31; }, nullptr, "cost_div 2^31");
  param_case([](P& p) { p.cost_div = (1u << 31) + 1; }, cd, "cost_div 2^31 + 1");
  param_case([](P& p) { p.cost_div = 0xFFFFFFFFu; }, cd, "cost_div 2^32 - 1");
  // the order within the parameters: the earlier field's message wins
  param_case([](P& p) { p.na = 0; p.nb = 0; }, na, "na before nb");
  param_case([](P& p) { p.nb = 0; p.opaque_mask = 0; }, nb, "nb before opaque_mask");
  param_case([](P& p) { p.na = 8192; p.nb = 8192; p.opaque_mask = 0; }, area, "area before opaque_mask");
  param_case([](P& p) { p.opaque_mask = 0; p.gain_mask = 0; }, om, "opaque_mask before gain_mask");
  param_case([](P& p) { p.gain_mask = 0; p.max_range = 0; }, gm, "gain_mask before max_range");
  param_case([](P& p) { p.max_range = 0; p.gain_weight = 0; }, mr, "max_range before gain_weight");
  param_case([](P& p) { p.gain_weight = 0; p.cost_div = 0; }, gw, "gain_weight before cost_div");
}

static void pointers() {
  const P p = good();
  P bad = good();
  bad.na = 0;
  P late = good();
  late.cost_div = 0;
  const O o = full();
  unsigned char* const ws = mem + 8;
  auto dev = [&](const void* cls, const void* views, int nv, const void* cost, const P* pp, const void* w, const O* oo, const void* counts,
                 const char* want, const char* where) {
    EXPECT(view_check(cls, views, nv, cost, pp, w, oo, counts, true, &err), want, where);
  };
  dev(mem, mem, 8, mem + 4, &p, ws, &o, mem + 8, nullptr, "everything given");
  dev(mem + 1, mem, 1, nullptr, &p, ws, &o, nullptr, nullptr, "an odd cls, no cost, no counts, one view");
  dev(mem, mem, 4096, nullptr, &p, ws, &o, nullptr, nullptr, "4096 views");
  dev(nullptr, mem, 8, mem, &p, ws, &o, nullptr, "grid_view: null cls", "null cls");
  dev(mem, mem, 8, mem, nullptr, ws, &o, nullptr, "grid_view: null params", "null params");
  dev(mem, nullptr, 8, mem, &p, ws, &o, nullptr, "grid_view: null views", "null views");
  dev(mem, mem, 8, mem, &p, nullptr, &o, nullptr, "grid_view: null workspace", "null workspace");
  dev(mem, mem, 8, mem, &p, ws, nullptr, nullptr, "grid_view: null out", "null out");
  // the nulls come in this order and before every range
  dev(nullptr, nullptr, 0, mem, nullptr, nullptr, nullptr, nullptr, "grid_view: null cls", "cls first");
  dev(mem, nullptr, 0, mem, nullptr, nullptr, nullptr, nullptr, "grid_view: null params", "params second");
  dev(mem, nullptr, 0, mem, &bad, nullptr, nullptr, nullptr, "grid_view: null views", "views third");
  dev(mem, mem, 0, mem, &bad, nullptr, nullptr, nullptr, "grid_view: null workspace", "workspace before the ranges");
  dev(mem, mem, 0, mem, &bad, ws, nullptr, nullptr, "grid_view: null out", "out before the ranges");
  dev(mem, mem, 0, mem, &bad, ws, &o, nullptr, "grid_view: na outside 1..8192", "then the ranges");
  const char* nvm = "grid_view: n_views outside 1..4096";
  dev(mem, mem, 0, mem, &late, ws, &o, nullptr, "grid_view: cost_div outside 1..2^31", "the last field before n_views");
  dev(mem, mem, 0, mem, &p, ws, &o, nullptr, nvm, "n_views 0");
  dev(mem, mem, 4097, mem, &p, ws, &o, nullptr, nvm, "n_views 4097");
  dev(mem, mem, -1, mem, &p, ws, &o, nullptr, nvm, "n_views -1");
  dev(mem, mem, INT_MIN, mem, &p, ws, &o, nullptr, nvm, "n_views INT_MIN");
  const char* all = "grid_view: records, order, best and seen are all null";
  O none{};
  dev(mem, mem, 8, mem, &p, ws, &none, nullptr, all, "no output");
  dev(mem, mem, 0, mem, &p, ws, &none, nullptr, nvm, "n_views before the outputs");
  dev(mem, mem + 1, 8, mem + 1, &p, ws, &none, nullptr, all, "the outputs before the alignments");
  for (int k = 0; k < 4; ++k) {  // each output alone is enough
    O one{};
    if (k == 0) one.records = o.records;
    if (k == 1) one.order = o.order;
    if (k == 2) one.best = o.best;
    if (k == 3) one.seen = o.seen;
    dev(mem, mem, 8, mem, &p, ws, &one, nullptr, nullptr, "one output");
  }
  const char *av = "grid_view: views must be 4-byte aligned", *ac = "grid_view: cost must be 4-byte aligned";
  const char *ao = "grid_view: order must be 4-byte aligned", *ab = "grid_view: best must be 4-byte aligned";
  const char *as = "grid_view: seen must be 4-byte aligned", *ar = "grid_view: records must be 8-byte aligned";
  const char *aw = "grid_view: workspace must be 8-byte aligned", *an = "grid_view: counts must be 8-byte aligned";
  O m = o;
  for (int off = 1; off < 4; ++off) dev(mem, mem + off, 8, mem, &p, ws, &o, nullptr, av, "views off 4");
  for (int off = 1; off < 4; ++off) dev(mem, mem, 8, mem + off, &p, ws, &o, nullptr, ac, "cost off 4");
  for (int off = 1; off < 4; ++off) { m = o; m.order = reinterpret_cast<uint32_t*>(mem + 64 + off); dev(mem, mem, 8, mem, &p, ws, &m, nullptr, ao, "order off 4"); }
  for (int off = 1; off < 4; ++off) { m = o; m.best = reinterpret_cast<uint32_t*>(mem + 128 + off); dev(mem, mem, 8, mem, &p, ws, &m, nullptr, ab, "best off 4"); }
  for (int off = 1; off < 4; ++off) { m = o; m.seen = reinterpret_cast<uint32_t*>(mem + 192 + off); dev(mem, mem, 8, mem, &p, ws, &m, nullptr, as, "seen off 4"); }
  for (int off = 1; off < 8; ++off) { m = o; m.records = reinterpret_cast<svo_grid_view_rec*>(mem + 16 + off); dev(mem, mem, 8, mem, &p, ws, &m, nullptr, ar, "records off 8"); }
  for (int off = 1; off < 8; ++off) dev(mem, mem, 8, mem, &p, ws + off, &o, nullptr, aw, "workspace off 8");
  for (int off = 1; off < 8; ++off) dev(mem, mem, 8, mem, &p, ws, &o, mem + 8 + off, an, "counts off 8");
  // their order: views, cost, order, best, seen, records, workspace, counts
  m = o; m.order = reinterpret_cast<uint32_t*>(mem + 65); m.best = reinterpret_cast<uint32_t*>(mem + 130); m.seen = reinterpret_cast<uint32_t*>(mem + 193);
  m.records = reinterpret_cast<svo_grid_view_rec*>(mem + 20);
  dev(mem, mem + 2, 8, mem + 2, &p, ws + 4, &m, mem + 4, av, "views first");
  dev(mem, mem, 8, mem + 2, &p, ws + 4, &m, mem + 4, ac, "cost second");
  dev(mem, mem, 8, mem, &p, ws + 4, &m, mem + 4, ao, "order third");
  m.order = o.order;
  dev(mem, mem, 8, mem, &p, ws + 4, &m, mem + 4, ab, "best fourth");
  m.best = o.best;
  dev(mem, mem, 8, mem, &p, ws + 4, &m, mem + 4, as, "seen fifth");
  m.seen = o.seen;
  dev(mem, mem, 8, mem, &p, ws + 4, &m, mem + 4, ar, "records sixth");
  m.records = o.records;
  dev(mem, mem, 8, mem, &p, ws + 4, &m, mem + 4, aw, "workspace seventh");
  dev(mem, mem, 8, mem, &p, ws, &m, mem + 4, an, "counts last");
  // the synchronous entry: no workspace, no alignment
  m = o; m.seen = reinterpret_cast<uint32_t*>(mem + 193); m.records = reinterpret_cast<svo_grid_view_rec*>(mem + 17);
  EXPECT(view_check(mem, mem + 1, 8, mem + 1, &p, nullptr, &m, mem + 3, false, &err), nullptr, "host pointers of any alignment");
  EXPECT(view_check(nullptr, mem, 8, nullptr, &p, nullptr, &m, nullptr, false, &err), "grid_view: null cls", "host: null cls");
  EXPECT(view_check(mem, mem, 8, nullptr, nullptr, nullptr, &m, nullptr, false, &err), "grid_view: null params", "host: null params");
  EXPECT(view_check(mem, nullptr, 8, nullptr, &p, nullptr, &m, nullptr, false, &err), "grid_view: null views", "host: null views");
  EXPECT(view_check(mem, mem, 8, nullptr, &p, nullptr, nullptr, nullptr, false, &err), "grid_view: null out", "host: null out");
  EXPECT(view_check(mem, mem, 0, nullptr, &p, nullptr, &m, nullptr, false, &err), nvm, "host: n_views 0");
  EXPECT(view_check(mem, mem, 8, nullptr, &p, nullptr, &none, nullptr, false, &err), all, "host: no output");
}

static size_t round8(size_t b) { return (b + 7) / 8 * 8; }

static void sizes() {
  struct Shape { int na, nb; };
  const Shape shapes[] = {{1, 1}, {1, 70}, {70, 1}, {17, 17}, {63, 65}, {130, 300}, {8192, 2048}, {2048, 8192}};
  for (const Shape& s : shapes)
    for (int nv : {1, 64, 4096}) {
      const size_t n = (size_t)s.na * (size_t)s.nb, bytes = view_workspace_bytes(s.na, s.nb, nv);
      CHECK(view_ws_slots_offset() == 256 && view_ws_seen_offset(nv) == 256 + 16 * (size_t)nv, "%d x %d, %d: layout", s.na, s.nb, nv);
      CHECK(bytes == 256 + 16 * (size_t)nv + round8(4 * n), "%d x %d, %d: the header's formula", s.na, s.nb, nv);
      CHECK(bytes % 8 == 0 && bytes >= view_ws_seen_offset(nv) + 4 * n && view_ws_seen_offset(nv) % 8 == 0, "%d x %d, %d: alignment and room", s.na, s.nb, nv);
    }
  CHECK(view_workspace_bytes(70000, 70000, 1) == 0 && view_workspace_bytes(0, 1, 1) == 0 && view_workspace_bytes(1, 0, 1) == 0 &&
            view_workspace_bytes(1, 1, 0) == 0 && view_workspace_bytes(1, 1, 4097) == 0 && view_workspace_bytes(8192, 2049, 1) == 0 &&
            view_workspace_bytes(-1, -1, -1) == 0,
        "refused shapes have no workspace");
  CHECK(view_workspace_bytes(1, 1, 1) == 256 + 16 + 8, "1 x 1, one view");
  // the window: rows of 2R + 1 bits in whole words, two planes
  const int ranges[] = {1, 2, 15, 16, 31, 32, 64, 255};
  const int words[] = {1, 1, 1, 2, 2, 3, 5, 16};
  for (int k = 0; k < 8; ++k) {
    const int r = ranges[k];
    CHECK(view_window_side(r) == 2 * r + 1 && view_window_row_words(r) == words[k] && view_window_plane_words(r) == (2 * r + 1) * words[k], "range %d: the window", r);
    CHECK(view_lds_bytes(r) == 8 * (size_t)(2 * r + 1) * (size_t)words[k] && view_lds_bytes(r) + 64 <= VIEW_LDS_LIMIT, "range %d: the LDS bytes", r);
    CHECK(view_targets(r) == (uint32_t)(2 * r + 1) * (uint32_t)(2 * r + 1) && view_target_rounds(r) == (view_targets(r) + 1023) / 1024, "range %d: targets", r);
  }
  CHECK(view_lds_bytes(255) == 65408 && view_lds_bytes(64) == 5160 && view_lds_bytes(0) == 0, "the LDS bytes at 255 and 64");
}

// every (da, db) with max(|da|, |db|) <= R exactly once; target 0 is V; ring n holds the targets of Chebyshev radius n, in this order
static void rings() {
  for (int R : {1, 2, 31, 32, 255}) {
    const int side = 2 * R + 1;
    std::vector<unsigned char> hit((size_t)side * side, 0);
    const uint32_t total = view_targets(R);
    int da = 7, db = 7;
    view_target_cell(0, &da, &db);
    CHECK(da == 0 && db == 0, "range %d: target 0 is V", R);
    uint32_t wrong = 0, twice = 0;
    for (uint32_t g = 0; g < total; ++g) {
      view_target_cell(g, &da, &db);
      const int n = abs(da) > abs(db) ? abs(da) : abs(db);
      if (n > R) { ++wrong; continue; }
      if (g > 0 && (view_ring_of(g) != n || g < view_ring_first(n) || g >= view_ring_first(n) + 8u * (uint32_t)n)) ++wrong;
      unsigned char& h = hit[(size_t)(da + R) * side + (size_t)(db + R)];
      twice += h;
      h = 1;
    }
    size_t visited = 0;
    for (unsigned char h : hit) visited += h;
    CHECK(wrong == 0 && twice == 0 && visited == (size_t)side * side, "range %d: %u wrong, %u twice, %zu of %zu visited", R, wrong, twice, visited, (size_t)side * side);
  }
  for (int n = 1; n <= 255; ++n) {
    CHECK(view_ring_first(n) == 1u + 4u * (uint32_t)n * (uint32_t)(n - 1) && view_ring_of(view_ring_first(n)) == n &&
              view_ring_of(view_ring_first(n) + 8u * (uint32_t)n - 1u) == n, "ring %d: first and last target", n);
    int da, db;
    view_ring_cell(n, 0, &da, &db);
    CHECK(da == -n && db == -n, "ring %d: position 0 is the corner (-n, -n)", n);
    view_ring_cell(n, 2 * n, &da, &db);
    CHECK(da == -n && db == n, "ring %d: position 2n is the corner (-n, +n)", n);
    view_ring_cell(n, 4 * n, &da, &db);
    CHECK(da == n && db == n, "ring %d: position 4n is the corner (+n, +n)", n);
    view_ring_cell(n, 8 * n - 1, &da, &db);
    CHECK(da == -n + 1 && db == -n, "ring %d: the last position", n);
  }
}

static void scores() {
  const uint32_t NONE = 0xFFFFFFFFu;
  CHECK(view_score(10, NONE, true, 16, 1) == 0, "unreachable");
  CHECK(view_score(10, NONE, false, 16, 1) == 160, "no cost field: the record's NONE is not a cost");
  CHECK(view_score(10, 100, true, 16, 1) == 60 && view_score(10, 160, true, 16, 1) == 0 && view_score(10, 161, true, 16, 1) == 0, "the cost below, at and above the gain");
  CHECK(view_score(10, 0xFFFFFFFEu, true, 16, 1) == 0, "a large cost does not wrap");
  CHECK(view_score(10, 1000, true, 16, 8) == 35 && view_score(10, 0xFFFFFFFEu, true, 16, 1u << 31) == 159, "cost_div");
  CHECK(view_score(65536, 0, true, 65536, 1) == 0xFFFFFFFEu && view_score(65535, 0, true, 65536, 1) == 0xFFFF0000u, "the clamp");
  CHECK(view_score(65536, 1, true, 65536, 1) == 0xFFFFFFFEu && view_score(65536, 2, true, 65536, 1) == 0xFFFFFFFEu && view_score(65536, 3, true, 65536, 1) == 0xFFFFFFFDu,
        "just under the clamp");
  CHECK(view_score(261121, 5, true, 65536, 1) == 0xFFFFFFFEu && view_score(0, 0, true, 65536, 1) == 0, "the largest gain, no gain");
}

static void defaults() {
  svo_grid_clearance_params c{};
  c.na = 256; c.nb = 300; c.source_mask = 4; c.max_dist = 64; c.cell_size = 0.5; c.inflate_radius = 0.0;
  P p{};
  CHECK(view_default_params(&c, &p) == SVO_OK, "defaults");
  CHECK(p.na == 256 && p.nb == 300 && p.opaque_mask == (1u << SVO_VOXEL_GRID_OBSTACLE) && p.gain_mask == (1u << SVO_VOXEL_GRID_UNKNOWN) &&
            p.max_range == 64 && p.gain_weight == 16 && p.cost_div == 1, "the defaults' values");
  EXPECT(view_params_check(&p, &err), nullptr, "the defaults pass the checks");
  c.max_dist = 255;
  CHECK(view_default_params(&c, &p) == SVO_OK && p.max_range == 255, "max_dist 255");
  c.max_dist = 256;
  CHECK(view_default_params(&c, &p) == SVO_OK && p.max_range == 255, "max_dist 256");
  c.max_dist = 8191;
  CHECK(view_default_params(&c, &p) == SVO_OK && p.max_range == 255, "max_dist 8191");
  c.max_dist = 1;
  CHECK(view_default_params(&c, &p) == SVO_OK && p.max_range == 1, "max_dist 1");
  CHECK(view_default_params(nullptr, &p) == SVO_ERR_INVALID && view_default_params(&c, nullptr) == SVO_ERR_INVALID, "null pointers");
  const P before = p;
  for (int k = 0; k < 5; ++k) {
    svo_grid_clearance_params b = c;
    if (k == 0) b.na = 0;
    if (k == 1) b.na = 8193;
    if (k == 2) b.nb = 0;
    if (k == 3) b.nb = 8193;
    if (k == 4) { b.na = 8192; b.nb = 2049; }
    CHECK(view_default_params(&b, &p) == SVO_ERR_INVALID && memcmp(&p, &before, sizeof(P)) == 0, "a refused clearance %d writes nothing", k);
  }
  c.na = 8192; c.nb = 2048;
  CHECK(view_default_params(&c, &p) == SVO_OK && p.na == 8192 && p.nb == 2048, "the largest grid");
}

int main() {
  params();
  pointers();
  sizes();
  rings();
  scores();
  defaults();
  if (fails) { fprintf(stderr, "%d check(s) failed\n", fails); return 1; }
  printf("grid view args ok\n");
  return 0;
}
