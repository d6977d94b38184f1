// The ground plan frontiers' GPU-free host logic (stereo_vo_amd/host/frontier_args.h) walked on the host, under ASan + UBSan: every
// refusal at its boundary with its code and its exact message and the accepted side of each boundary, the order of the refusals, the
// workspace's size, layout and bound, the tile, seam-cell and scan-block counts at 1 x 1, T - 1, T, T + 1, 8192 x 2048 and past 2^32,
// the defaults.
#include <limits.h>
#include <stdio.h>
#include <string.h>

#include <initializer_list>

#include "frontier_args.h"

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { ++fails; fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

// rc is the refusal with exactly this message, or (want == nullptr) SVO_OK with the message untouched
static void expect(int rc, const char* err, const char* want, const char* where) {
  if (want) CHECK(rc == SVO_ERR_INVALID && err && strcmp(err, want) == 0, "%s: rc %d, message '%s', wanted '%s'", where, rc, err ? err : "(none)", want);
  else CHECK(rc == SVO_OK && err == nullptr, "%s: rc %d, message '%s', wanted acceptance", where, rc, err ? err : "(none)");
}

// the check runs first: its message is read only after it returned
#define EXPECT(call, want, where) do { const char* err = nullptr; const int rc_ = (call); expect(rc_, err, want, where); } while (0)

using P = svo_grid_frontier_params;
using O = svo_grid_frontier_out;
constexpr int T = FRONTIER_TILE;

static P good() {
  P p;
  p.na = 32; p.nb = 13; p.free_mask = 2u; p.unknown_mask = 1u; p.min_size = 3; p.max_frontiers = 1024;
  return p;
}

alignas(16) static unsigned char mem[256];
static O full() {
  O o;
  o.frontiers = reinterpret_cast<svo_grid_frontier*>(mem + 16); o.goal_cells = reinterpret_cast<uint32_t*>(mem + 64); o.label = reinterpret_cast<uint32_t*>(mem + 128);
  return o;
}

template <typename F>
static void param_case(F change, const char* want, const char* where) {
  P p = good();
  change(p);
  EXPECT(frontier_params_check(&p, &err), want, where);
  const O o = full();
  EXPECT(frontier_check(mem, mem + 4, &p, mem + 8, &o, mem + 8, true, &err), want, where);
  EXPECT(frontier_check(mem, mem + 1, &p, nullptr, &o, mem + 1, false, &err), want, where);
  CHECK((frontier_workspace_bytes(p.na, p.nb, p.max_frontiers) == 0) ==
            (p.na < 1 || p.na > 8192 || p.nb < 1 || p.nb > 8192 || (long long)p.na * p.nb > (1ll << 24) || p.max_frontiers < 1 || p.max_frontiers > 65536),
        "%s: the workspace is 0 exactly for a refused shape or max_frontiers", where);
}

static void params() {
  const char *na = "grid_frontier: na outside 1..8192", *nb = "grid_frontier: nb outside 1..8192", *area = "grid_frontier: na * nb beyond 2^24";
  const char *fm = "grid_frontier: free_mask is 0", *um = "grid_frontier: unknown_mask is 0", *ms = "grid_frontier: min_size outside 1..2^24";
  const char *mf = "grid_frontier: max_frontiers outside 1..65536", *share = "grid_frontier: free_mask and unknown_mask share a bit";
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
  param_case([](P& p) { p.free_mask = 0; }, fm, "free_mask 0");
  param_case([](P& p) { p.free_mask = 0x80000000u; }, nullptr, "free_mask bit 31");
  param_case([](P& p) { p.unknown_mask = 0; }, um, "unknown_mask 0");
  param_case([](P& p) { p.free_mask = 0xFFFFFFFEu; }, nullptr, "every other class free");
  param_case([](P& p) { p.min_size = 0; }, ms, "min_size 0");
  param_case([](P& p) { p.min_size = 1; }, nullptr, "min_size 1");
  param_case([](P& p) { p.min_size = 1u << 24; }, nullptr, "min_size 2^24");
  param_case([](P& p) { p.min_size = (1u << 24) + 1; }, ms, "min_size 2^24 + 1");
  param_case([](P& p) { p.min_size = 0xFFFFFFFFu; }, ms, "min_size 2^32 - 1");
  param_case([](P& p) { p.max_frontiers = 0; }, mf, "max_frontiers 0");
  param_case([](P& p) { p.max_frontiers = 1; }, nullptr, "max_frontiers 1");
  param_case([](P& p) { p.max_frontiers = 65536; }, nullptr, "max_frontiers 65536");
  param_case([](P& p) { p.max_frontiers = 65537; }, mf, "max_frontiers 65537");
  param_case([](P& p) { p.max_frontiers = -1; }, mf, "max_frontiers -1");
  param_case([](P& p) { p.free_mask = 3u; }, share, "bit 0 in both");
  param_case([](P& p) { p.free_mask = 0x80000002u; p.unknown_mask = 0x80000001u; }, share, "bit 31 in both");
  // the order within the parameters: the earlier field's message wins
  param_case([](P& p) { p.na = 0; p.nb = 0; }, na, "na before nb");
  param_case([](P& p) { p.nb = 0; p.free_mask = 0; }, nb, "nb before free_mask");
  param_case([](P& p) { p.na = 8192; p.nb = 8192; p.free_mask = 0; }, area, "area before free_mask");
  param_case([](P& p) { p.free_mask = 0; p.unknown_mask = 0; }, fm, "free_mask before unknown_mask");
  param_case([](P& p) { p.unknown_mask = 0; p.min_size = 0; }, um, "unknown_mask before min_size");
  param_case([](P& p) { p.min_size = 0; p.max_frontiers = 0; }, ms, "min_size before max_frontiers");
  param_case([](P& p) { p.max_frontiers = 0; p.free_mask = 3u; }, mf, "max_frontiers before the common bit");
}

static void pointers() {
  const P p = good();
  P bad = good();
  bad.na = 0;
  const O o = full();
  unsigned char* const ws = mem + 8;
  auto dev = [&](const void* cls, const void* cost, const P* pp, const void* w, const O* oo, const void* counts, const char* want, const char* where) {
    EXPECT(frontier_check(cls, cost, pp, w, oo, counts, true, &err), want, where);
  };
  dev(mem, mem + 4, &p, ws, &o, mem + 8, nullptr, "everything given");
  dev(mem + 1, nullptr, &p, ws, &o, nullptr, nullptr, "an odd cls, no cost, no counts");
  dev(nullptr, mem, &p, ws, &o, nullptr, "grid_frontier: null cls", "null cls");
  dev(mem, mem, nullptr, ws, &o, nullptr, "grid_frontier: null params", "null params");
  dev(mem, mem, &p, nullptr, &o, nullptr, "grid_frontier: null workspace", "null workspace");
  dev(mem, mem, &p, ws, nullptr, nullptr, "grid_frontier: null out", "null out");
  // the nulls come in this order and before every range
  dev(nullptr, mem, nullptr, nullptr, nullptr, nullptr, "grid_frontier: null cls", "cls first");
  dev(mem, mem, nullptr, nullptr, nullptr, nullptr, "grid_frontier: null params", "params second");
  dev(mem, mem, &bad, nullptr, nullptr, nullptr, "grid_frontier: null workspace", "workspace before the ranges");
  dev(mem, mem, &bad, ws, nullptr, nullptr, "grid_frontier: null out", "out before the ranges");
  dev(mem, mem, &bad, ws, &o, nullptr, "grid_frontier: na outside 1..8192", "then the ranges");
  const char* all = "grid_frontier: frontiers, goal_cells and label are all null";
  O none{};
  dev(mem, mem, &p, ws, &none, nullptr, all, "no output");
  P sh = good();
  sh.free_mask = 3u;
  dev(mem, mem, &sh, ws, &none, nullptr, "grid_frontier: free_mask and unknown_mask share a bit", "the common bit before the outputs");
  dev(mem, mem + 1, &p, ws, &none, nullptr, all, "the outputs before the alignments");
  for (int k = 0; k < 3; ++k) {  // each output alone is enough
    O one{};
    if (k == 0) one.frontiers = o.frontiers;
    if (k == 1) one.goal_cells = o.goal_cells;
    if (k == 2) one.label = o.label;
    dev(mem, mem, &p, ws, &one, nullptr, nullptr, "one output");
  }
  const char *ac = "grid_frontier: cost must be 4-byte aligned", *al = "grid_frontier: label must be 4-byte aligned";
  const char *ag = "grid_frontier: goal_cells must be 4-byte aligned", *af = "grid_frontier: frontiers must be 8-byte aligned";
  const char *aw = "grid_frontier: workspace must be 8-byte aligned", *an = "grid_frontier: counts must be 8-byte aligned";
  O m = o;
  for (int off = 1; off < 4; ++off) dev(mem, mem + off, &p, ws, &o, nullptr, ac, "cost off 4");
  for (int off = 1; off < 4; ++off) { m = o; m.label = reinterpret_cast<uint32_t*>(mem + 128 + off); dev(mem, mem, &p, ws, &m, nullptr, al, "label off 4"); }
  for (int off = 1; off < 4; ++off) { m = o; m.goal_cells = reinterpret_cast<uint32_t*>(mem + 64 + off); dev(mem, mem, &p, ws, &m, nullptr, ag, "goal_cells off 4"); }
  for (int off = 1; off < 8; ++off) { m = o; m.frontiers = reinterpret_cast<svo_grid_frontier*>(mem + 16 + off); dev(mem, mem, &p, ws, &m, nullptr, af, "frontiers off 8"); }
  for (int off = 1; off < 8; ++off) dev(mem, mem, &p, ws + off, &o, nullptr, aw, "workspace off 8");
  for (int off = 1; off < 8; ++off) dev(mem, mem, &p, ws, &o, mem + 8 + off, an, "counts off 8");
  // their order: cost, label, goal_cells, frontiers, workspace, counts
  m = o; m.label = reinterpret_cast<uint32_t*>(mem + 129); m.goal_cells = reinterpret_cast<uint32_t*>(mem + 65); m.frontiers = reinterpret_cast<svo_grid_frontier*>(mem + 20);
  dev(mem, mem + 2, &p, ws + 4, &m, mem + 4, ac, "cost first");
  dev(mem, mem, &p, ws + 4, &m, mem + 4, al, "label second");
  m.label = o.label;
  dev(mem, mem, &p, ws + 4, &m, mem + 4, ag, "goal_cells third");
  m.goal_cells = o.goal_cells;
  dev(mem, mem, &p, ws + 4, &m, mem + 4, af, "frontiers fourth");
  m.frontiers = o.frontiers;
  dev(mem, mem, &p, ws + 4, &m, mem + 4, aw, "workspace fifth");
  dev(mem, mem, &p, ws, &m, mem + 4, an, "counts last");
  // the synchronous entry: no workspace, no alignment
  m = o; m.label = reinterpret_cast<uint32_t*>(mem + 129); m.frontiers = reinterpret_cast<svo_grid_frontier*>(mem + 17);
  EXPECT(frontier_check(mem, mem + 1, &p, nullptr, &m, mem + 3, false, &err), nullptr, "host pointers of any alignment");
  EXPECT(frontier_check(nullptr, nullptr, &p, nullptr, &m, nullptr, false, &err), "grid_frontier: null cls", "host: null cls");
  EXPECT(frontier_check(mem, nullptr, nullptr, nullptr, &m, nullptr, false, &err), "grid_frontier: null params", "host: null params");
  EXPECT(frontier_check(mem, nullptr, &p, nullptr, nullptr, nullptr, false, &err), "grid_frontier: null out", "host: null out");
  EXPECT(frontier_check(mem, nullptr, &p, nullptr, &none, nullptr, false, &err), all, "host: no output");
}

static size_t round8(size_t b) { return (b + 7) / 8 * 8; }

static void sizes_and_geometry() {
  struct Shape { int na, nb; };
  const Shape shapes[] = {{1, 1}, {T - 1, T - 1}, {T, T}, {T + 1, T + 1}, {1, 257}, {257, 1}, {T, T + 1}, {T + 1, T}, {130, 300}, {8192, 2048}, {2048, 8192}};
  for (const Shape& s : shapes)
    for (int mf : {1, 64, 1024, 65536}) {
      const size_t n = (size_t)s.na * (size_t)s.nb, ta = ((size_t)s.na + T - 1) / T, tb = ((size_t)s.nb + T - 1) / T, blocks = (n + 255) / 256;
      CHECK(frontier_tiles_along(s.na) == ta && frontier_tiles(s.na, s.nb) == ta * tb, "%d x %d: tiles", s.na, s.nb);
      CHECK(frontier_seam_cols(s.na, s.nb) == (tb - 1) * (size_t)s.na && frontier_seam_rows(s.na, s.nb) == (ta - 1) * (size_t)s.nb &&
                frontier_seam_cells(s.na, s.nb) == (tb - 1) * (size_t)s.na + (ta - 1) * (size_t)s.nb, "%d x %d: seam cells", s.na, s.nb);
      // by counting: the cells whose column, or whose row, is a positive multiple of T
      if (n <= 100000) {
        size_t cols = 0, rows = 0;
        for (int ia = 0; ia < s.na; ++ia)
          for (int ib = 0; ib < s.nb; ++ib) { cols += ib > 0 && ib % T == 0; rows += ia > 0 && ia % T == 0; }
        CHECK(cols == frontier_seam_cols(s.na, s.nb) && rows == frontier_seam_rows(s.na, s.nb), "%d x %d: seam cells by counting", s.na, s.nb);
      }
      CHECK(frontier_scan_blocks(s.na, s.nb) == blocks && blocks <= 65536 && frontier_groups(n) == blocks, "%d x %d: scan blocks", s.na, s.nb);
      const size_t o_slots = frontier_ws_slots_offset(), o_blocks = frontier_ws_blocks_offset(mf), o_parent = frontier_ws_cells_offset(0, s.na, s.nb, mf),
                   o_size = frontier_ws_cells_offset(1, s.na, s.nb, mf), o_rank = frontier_ws_cells_offset(2, s.na, s.nb, mf),
                   o_end = frontier_ws_cells_offset(3, s.na, s.nb, mf), bytes = frontier_workspace_bytes(s.na, s.nb, mf);
      CHECK(o_slots == 256 && o_blocks == 256 + 64 * (size_t)mf && o_parent == o_blocks + round8(4 * blocks) && o_size == o_parent + 4 * n &&
                o_rank == o_size + 4 * n && o_end == o_rank + 4 * n, "%d x %d, %d: layout", s.na, s.nb, mf);
      CHECK(bytes == 256 + 64 * (size_t)mf + round8(4 * blocks) + round8(12 * n), "%d x %d, %d: the header's formula", s.na, s.nb, mf);
      CHECK(bytes % 8 == 0 && bytes >= o_end && bytes < o_end + 8, "%d x %d, %d: rounded up to 8", s.na, s.nb, mf);
      CHECK(o_slots % 8 == 0 && o_blocks % 8 == 0 && o_parent % 8 == 0 && o_size % 4 == 0 && o_rank % 4 == 0, "%d x %d, %d: alignment", s.na, s.nb, mf);
      CHECK(bytes <= 16 * n + 64 * (size_t)mf + 4096, "%d x %d, %d: the contract's bound", s.na, s.nb, mf);
    }
  CHECK(frontier_groups(0) == 0 && frontier_groups(1) == 1 && frontier_groups(256) == 1 && frontier_groups(257) == 2, "groups");
  CHECK(frontier_tiles_along(0) == 0 && frontier_tiles_along(-5) == 0 && frontier_tiles_along(INT_MAX) == ((size_t)INT_MAX + T - 1) / T, "tiles along at the ends");
  CHECK(frontier_seam_cells(0, 5) == 0 && frontier_seam_cells(5, 0) == 0 && frontier_scan_blocks(0, 5) == 0 && frontier_scan_blocks(-1, -1) == 0, "empty shapes");
  // past 2^32: computed in size_t, no wrap (such a shape is refused; the helpers still count right)
  if (sizeof(size_t) >= 8) {
    const size_t n = (size_t)70000 * 70000;
    CHECK(frontier_scan_blocks(70000, 70000) == (n + 255) / 256, "scan blocks past 2^32");
    CHECK(frontier_ws_cells_offset(3, 70000, 70000, 1) == 256 + 64 + round8(4 * ((n + 255) / 256)) + 12 * n, "offsets past 2^32");
    CHECK(frontier_tiles(INT_MAX, INT_MAX) == (((size_t)INT_MAX + T - 1) / T) * (((size_t)INT_MAX + T - 1) / T), "tiles past 2^32");
  }
  CHECK(frontier_workspace_bytes(70000, 70000, 1) == 0 && frontier_workspace_bytes(0, 1, 1) == 0 && frontier_workspace_bytes(1, 0, 1) == 0 &&
            frontier_workspace_bytes(1, 1, 0) == 0 && frontier_workspace_bytes(1, 1, 65537) == 0 && frontier_workspace_bytes(8192, 2049, 1) == 0,
        "refused shapes have no workspace");
  CHECK(frontier_workspace_bytes(1, 1, 1) == 256 + 64 + 8 + 16, "1 x 1, one record");
}

static void defaults() {
  svo_grid_clearance_params c{};
  c.na = 256; c.nb = 300; c.source_mask = 4; c.max_dist = 64; c.cell_size = 0.5; c.inflate_radius = 0.0;
  P p{};
  CHECK(frontier_default_params(&c, &p) == SVO_OK, "defaults");
  CHECK(p.na == 256 && p.nb == 300 && p.free_mask == (1u << SVO_VOXEL_GRID_LEVEL) && p.unknown_mask == (1u << SVO_VOXEL_GRID_UNKNOWN) &&
            p.min_size == 3 && p.max_frontiers == 1024, "the defaults' values");
  EXPECT(frontier_params_check(&p, &err), nullptr, "the defaults pass the checks");
  CHECK(frontier_default_params(nullptr, &p) == SVO_ERR_INVALID && frontier_default_params(&c, nullptr) == SVO_ERR_INVALID, "null pointers");
  const P before = p;
  for (int k = 0; k < 5; ++k) {
    svo_grid_clearance_params b = c;
    if (k == 0) b.na = 0;
    if (k == 1) b.na = 8193;
    if (k == 2) b.nb = 0;
    if (k == 3) b.nb = 8193;
    if (k == 4) { b.na = 8192; b.nb = 2049; }
    CHECK(frontier_default_params(&b, &p) == SVO_ERR_INVALID && memcmp(&p, &before, sizeof(P)) == 0, "a refused clearance %d writes nothing", k);
  }
  c.na = 8192; c.nb = 2048;
  CHECK(frontier_default_params(&c, &p) == SVO_OK && p.na == 8192 && p.nb == 2048, "the largest grid");
}

int main() {
  params();
  pointers();
  sizes_and_geometry();
  defaults();
  if (fails) { fprintf(stderr, "%d check(s) failed\n", fails); return 1; }
  printf("grid frontier args ok\n");
  return 0;
}
