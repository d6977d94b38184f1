// The ground plan waypoints' GPU-free host logic (stereo_vo_amd/host/waypoint_args.h) walked on the host, under ASan + UBSan: every
// refusal at its boundary with its code and its exact message and the accepted side of each boundary, the order of the refusals, the
// line stepper against rule 3's closed formula for every (da, db) with |d| <= 255, CLEAR on hand-made corners over a small grid whose
// look-up fails on a cell outside the bounding box of V and T, the defaults.
#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "waypoint_args.h"

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { ++fails; fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

// rc is the refusal with exactly this message, or (want == nullptr) SVO_OK with the message untouched
static void expect(int rc, const char* err, const char* want, const char* where) {
  if (want) CHECK(rc == SVO_ERR_INVALID && err && strcmp(err, want) == 0, "%s: rc %d, message '%s', wanted '%s'", where, rc, err ? err : "(none)", want);
  else CHECK(rc == SVO_OK && err == nullptr, "%s: rc %d, message '%s', wanted acceptance", where, rc, err ? err : "(none)");
}

// the check runs first: its message is read only after it returned
#define EXPECT(call, want, where) do { const char* err = nullptr; const int rc_ = (call); expect(rc_, err, want, where); } while (0)

using P = svo_grid_waypoint_params;
using O = svo_grid_waypoint_out;

static P good() {
  P p;
  p.na = 32; p.nb = 13; p.path_stride = 64; p.max_look = 64; p.min_dist2 = 0u; p.max_way = 16; p.cell_size = 0.25;
  return p;
}

alignas(16) static unsigned char mem[512];
static O full() {
  O o;
  o.way = reinterpret_cast<uint32_t*>(mem + 16); o.way_index = reinterpret_cast<uint32_t*>(mem + 64);
  o.way_len = reinterpret_cast<uint32_t*>(mem + 128); o.way_status = mem + 193; o.length = reinterpret_cast<double*>(mem + 256);
  return o;
}

template <typename F>
static void param_case(F change, const char* want, const char* where) {
  P p = good();
  change(p);
  EXPECT(way_params_check(&p, &err), want, where);
  const O o = full();
  EXPECT(way_check(mem, mem + 4, mem + 4, mem + 4, 8, &p, &o, mem + 8, true, &err), want, where);
  EXPECT(way_check(mem, mem + 1, mem + 1, mem + 1, 8, &p, &o, mem + 1, false, &err), want, where);
}

static void params() {
  const char *na = "grid_waypoints: na outside 1..8192", *nb = "grid_waypoints: nb outside 1..8192", *area = "grid_waypoints: na * nb beyond 2^24";
  const char *ps = "grid_waypoints: path_stride outside 1..2^20", *ml = "grid_waypoints: max_look outside 1..255";
  const char *md = "grid_waypoints: min_dist2 beyond 2^26", *mw = "grid_waypoints: max_way outside 1..2^20";
  const char *cs = "grid_waypoints: cell_size must be finite and > 0";
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
  param_case([](P& p) { p.na = 8192; p.nb = 2049; }, area, "2^24 + 8192 cells");
  param_case([](P& p) { p.na = 8192; p.nb = 8192; }, area, "2^26 cells");
  param_case([](P& p) { p.path_stride = 0; }, ps, "path_stride 0");
  param_case([](P& p) { p.path_stride = 1; }, nullptr, "path_stride 1");
  param_case([](P& p) { p.path_stride = 1 << 20; }, nullptr, "path_stride 2^20");
  param_case([](P& p) { p.path_stride = (1 << 20) + 1; }, ps, "path_stride 2^20 + 1");
  param_case([](P& p) { p.path_stride = INT_MIN; }, ps, "path_stride INT_MIN");
  param_case([](P& p) { p.max_look = 0; }, ml, "max_look 0");
  param_case([](P& p) { p.max_look = 1; }, nullptr, "max_look 1");
  param_case([](P& p) { p.max_look = 255; }, nullptr, "max_look 255");
  param_case([](P& p) { p.max_look = 256; }, ml, "max_look 256");
  param_case([](P& p) { p.max_look = -1; }, ml, "max_look -1");
  param_case([](P& p) { p.min_dist2 = 1u << 26; }, nullptr, "min_dist2 2^26");
  param_case([](P& p) { p.min_dist2 = (1u << 26) + 1u; }, md, "min_dist2 2^26 + 1");
  param_case([](P& p) { p.min_dist2 = 0xFFFFFFFFu; }, md, "min_dist2 all ones");
  param_case([](P& p) { p.max_way = 0; }, mw, "max_way 0");
  param_case([](P& p) { p.max_way = 1; }, nullptr, "max_way 1");
  param_case([](P& p) { p.max_way = 1 << 20; }, nullptr, "max_way 2^20");
  param_case([](P& p) { p.max_way = (1 << 20) + 1; }, mw, "max_way 2^20 + 1");
  param_case([](P& p) { p.max_way = INT_MAX; }, mw, "max_way INT_MAX");
  param_case([](P& p) { p.cell_size = 0.0; }, cs, "cell_size 0");
  param_case([](P& p) { p.cell_size = -0.5; }, cs, "cell_size -0.5");
  param_case([](P& p) { p.cell_size = INFINITY; }, cs, "cell_size inf");
  param_case([](P& p) { p.cell_size = NAN; }, cs, "cell_size nan");
  param_case([](P& p) { p.cell_size = 5e-324; }, nullptr, "cell_size denormal");
  param_case([](P& p) { p.cell_size = DBL_MAX; }, nullptr, "cell_size DBL_MAX");
  // the order of the fields
  param_case([](P& p) { p.na = 0; p.nb = 0; }, na, "na before nb");
  param_case([](P& p) { p.nb = 0; p.path_stride = 0; }, nb, "nb before path_stride");
  param_case([](P& p) { p.na = 8192; p.nb = 8192; p.path_stride = 0; }, area, "the area before path_stride");
  param_case([](P& p) { p.path_stride = 0; p.max_look = 0; }, ps, "path_stride before max_look");
  param_case([](P& p) { p.max_look = 0; p.min_dist2 = 0xFFFFFFFFu; }, ml, "max_look before min_dist2");
  param_case([](P& p) { p.min_dist2 = 0xFFFFFFFFu; p.max_way = 0; }, md, "min_dist2 before max_way");
  param_case([](P& p) { p.max_way = 0; p.cell_size = 0.0; }, mw, "max_way before cell_size");
}

static void pointers() {
  const P p = good();
  P bad = good();
  bad.na = 0;
  const O o = full();
  unsigned char* const b = mem;
  EXPECT(way_check(b, b + 4, b + 4, b + 4, 1, &p, &o, b + 8, true, &err), nullptr, "all good");
  EXPECT(way_check(b, nullptr, b + 4, b + 4, 4096, &p, &o, nullptr, true, &err), nullptr, "no dist2, no counts, 4096 paths");
  EXPECT(way_check(nullptr, b + 4, b + 4, b + 4, 1, &p, &o, b + 8, true, &err), "grid_waypoints: null blocked", "null blocked");
  EXPECT(way_check(b, b + 4, b + 4, b + 4, 1, nullptr, &o, b + 8, true, &err), "grid_waypoints: null params", "null params");
  EXPECT(way_check(b, b + 4, nullptr, b + 4, 1, &p, &o, b + 8, true, &err), "grid_waypoints: null path", "null path");
  EXPECT(way_check(b, b + 4, b + 4, nullptr, 1, &p, &o, b + 8, true, &err), "grid_waypoints: null path_len", "null path_len");
  EXPECT(way_check(b, b + 4, b + 4, b + 4, 1, &p, nullptr, b + 8, true, &err), "grid_waypoints: null out", "null out");
  EXPECT(way_check(nullptr, b + 4, nullptr, nullptr, 1, nullptr, nullptr, b + 8, true, &err), "grid_waypoints: null blocked", "blocked first");
  EXPECT(way_check(b, b + 4, nullptr, nullptr, 1, nullptr, nullptr, b + 8, true, &err), "grid_waypoints: null params", "params second");
  EXPECT(way_check(b, b + 4, nullptr, nullptr, 1, &p, nullptr, b + 8, true, &err), "grid_waypoints: null path", "path third");
  EXPECT(way_check(b, b + 4, b + 4, nullptr, 1, &p, nullptr, b + 8, true, &err), "grid_waypoints: null path_len", "path_len fourth");
  EXPECT(way_check(b, b + 4, b + 4, b + 4, 1, &bad, nullptr, b + 8, true, &err), "grid_waypoints: null out", "the nulls before the ranges");
  const char* np = "grid_waypoints: n_paths outside 1..4096";
  EXPECT(way_check(b, b + 4, b + 4, b + 4, 0, &p, &o, b + 8, true, &err), np, "n_paths 0");
  EXPECT(way_check(b, b + 4, b + 4, b + 4, 4097, &p, &o, b + 8, true, &err), np, "n_paths 4097");
  EXPECT(way_check(b, b + 4, b + 4, b + 4, INT_MIN, &p, &o, b + 8, false, &err), np, "n_paths INT_MIN");
  P late = good();
  late.cell_size = 0.0;
  EXPECT(way_check(b, b + 4, b + 4, b + 4, 0, &late, &o, b + 8, true, &err), "grid_waypoints: cell_size must be finite and > 0", "the fields before n_paths");
  const char *together = "grid_waypoints: way and way_len go together", *none = "grid_waypoints: every output is null";
  O q = full(); q.way = nullptr;
  EXPECT(way_check(b, b + 4, b + 4, b + 4, 1, &p, &q, b + 8, true, &err), together, "way_len without way");
  EXPECT(way_check(b, b + 4, b + 4, b + 4, 0, &p, &q, b + 8, true, &err), np, "n_paths before the outputs' rules");
  q = full(); q.way_len = nullptr;
  EXPECT(way_check(b, b + 4, b + 4, b + 4, 1, &p, &q, b + 8, false, &err), together, "way without way_len");
  q = O{};
  EXPECT(way_check(b, b + 4, b + 4, b + 4, 1, &p, &q, b + 8, true, &err), none, "no output");
  EXPECT(way_check(b, b + 4, b + 4, b + 4, 1, &p, &q, b + 8, false, &err), none, "no output, host");
  for (int k = 0; k < 3; ++k) {  // each of the single outputs alone
    q = O{};
    if (k == 0) q.way_index = full().way_index; else if (k == 1) q.way_status = full().way_status; else q.length = full().length;
    EXPECT(way_check(b, b + 4, b + 4, b + 4, 1, &p, &q, b + 8, true, &err), nullptr, "one output alone");
  }
  q = O{}; q.way = full().way; q.way_len = full().way_len;
  EXPECT(way_check(b, b + 4, b + 4, b + 4, 1, &p, &q, b + 8, true, &err), nullptr, "way and way_len alone");
  // the alignments, the device entry's alone, 4 bytes before 8 and in the order of the list
  q = full(); q.way = nullptr;
  EXPECT(way_check(b, b + 2, b + 4, b + 4, 1, &p, &q, b + 8, true, &err), together, "the outputs' rules before the alignments");
  const char* names4[6] = {"dist2", "path", "path_len", "way", "way_index", "way_len"};
  for (int k = 0; k < 6; ++k) {
    char want[96];
    snprintf(want, sizeof want, "grid_waypoints: %s must be 4-byte aligned", names4[k]);
    for (int off = 1; off <= 3; ++off) {
      q = full();
      const unsigned char *d2 = b + 4, *pa = b + 4, *pl = b + 4;
      if (k == 0) d2 += off; else if (k == 1) pa += off; else if (k == 2) pl += off;
      else if (k == 3) q.way = reinterpret_cast<uint32_t*>(mem + 16 + off);
      else if (k == 4) q.way_index = reinterpret_cast<uint32_t*>(mem + 64 + off);
      else q.way_len = reinterpret_cast<uint32_t*>(mem + 128 + off);
      EXPECT(way_check(b, d2, pa, pl, 1, &p, &q, b + 8, true, &err), want, names4[k]);
      EXPECT(way_check(b, d2, pa, pl, 1, &p, &q, b + 8, false, &err), nullptr, "the host entry asks no alignment");
      // every later pointer off as well: the first in the list is named
      O r = q;
      if (k < 5) r.way_len = reinterpret_cast<uint32_t*>(mem + 129);
      r.length = reinterpret_cast<double*>(mem + 260);
      EXPECT(way_check(b, d2, pa, pl, 1, &p, &r, b + 12, true, &err), want, "the first misaligned pointer is named");
    }
  }
  q = full(); q.length = reinterpret_cast<double*>(mem + 260);
  EXPECT(way_check(b, b + 4, b + 4, b + 4, 1, &p, &q, b + 8, true, &err), "grid_waypoints: length must be 8-byte aligned", "length off 8");
  EXPECT(way_check(b, b + 4, b + 4, b + 4, 1, &p, &q, b + 12, true, &err), "grid_waypoints: length must be 8-byte aligned", "length before counts");
  q = full();
  EXPECT(way_check(b, b + 4, b + 4, b + 4, 1, &p, &q, b + 12, true, &err), "grid_waypoints: counts must be 8-byte aligned", "counts off 8");
  EXPECT(way_check(b + 1, b + 4, b + 4, b + 4, 1, &p, &q, b + 8, true, &err), nullptr, "blocked and way_status are bytes");
}

// rule 3's closed formula
static void closed(int da, int db, int i, int* oa, int* ob) {
  const int ada = abs(da), adb = abs(db), n = ada > adb ? ada : adb;
  const int sa = (da > 0) - (da < 0), sb = (db > 0) - (db < 0);
  *oa = sa * ((2 * i * ada + n) / (2 * n));
  *ob = sb * ((2 * i * adb + n) / (2 * n));
}

static void lines() {
  long long steps = 0;
  for (int da = -255; da <= 255; ++da)
    for (int db = -255; db <= 255; ++db) {
      WayLine l = way_line(da, db);
      const int n = abs(da) > abs(db) ? abs(da) : abs(db);
      if (l.n != n || l.pa != 0 || l.pb != 0) { CHECK(false, "line (%d, %d): n %d, start (%d, %d)", da, db, l.n, l.pa, l.pb); return; }
      for (int i = 1; i <= n; ++i) {
        way_line_step(&l);
        int oa, ob;
        closed(da, db, i, &oa, &ob);
        ++steps;
        if (l.sa * l.pa != oa || l.sb * l.pb != ob) { CHECK(false, "line (%d, %d) step %d: (%d, %d), the formula says (%d, %d)", da, db, i, l.sa * l.pa, l.sb * l.pb, oa, ob); return; }
      }
      if (n && (l.sa * l.pa != da || l.sb * l.pb != db)) { CHECK(false, "line (%d, %d) does not end at T", da, db); return; }
    }
  CHECK(steps == 44477440ll, "every step of every line was compared: %lld", steps);
  // a tie of the minor coordinate rounds away from V: (0,0) -> (2,1) passes (1,1), and (2,1) -> (0,0) passes (1,0)
  WayLine l = way_line(2, 1);
  way_line_step(&l);
  CHECK(l.pa == 1 && l.pb == 1, "the tie from V: (%d, %d)", l.pa, l.pb);
  l = way_line(-2, -1);
  way_line_step(&l);
  CHECK(l.sa * l.pa == -1 && l.sb * l.pb == -1, "the tie from T: (%d, %d)", l.sa * l.pa, l.sb * l.pb);
}

// A small grid whose look-up counts its calls and fails on a cell outside the bounding box it was told.
struct Grid {
  int na, nb;
  std::vector<unsigned char> solid;
  mutable int a0, a1, b0, b1, asked;
  bool operator()(int ia, int ib) const {
    ++asked;
    if (ia < a0 || ia > a1 || ib < b0 || ib > b1) { ++fails; fprintf(stderr, "FAIL: (%d, %d) asked outside the box of V and T\n", ia, ib); return true; }
    return solid.at((size_t)ia * nb + ib) != 0;
  }
};

static bool clear(const Grid& g, int va, int vb, int ta, int tb, int look) {
  g.a0 = va < ta ? va : ta; g.a1 = va < ta ? ta : va; g.b0 = vb < tb ? vb : tb; g.b1 = vb < tb ? tb : vb; g.asked = 0;
  return way_clear(va, vb, ta, tb, look, g);
}

static void corners() {
  Grid g{9, 9, std::vector<unsigned char>(81, 0), 0, 0, 0, 0, 0};
  auto set = [&](int a, int b, int v) { g.solid[(size_t)a * 9 + b] = (unsigned char)v; };
  CHECK(clear(g, 4, 4, 4, 4, 1), "n = 0 on open ground");
  CHECK(clear(g, 0, 0, 8, 8, 8) && !clear(g, 0, 0, 8, 8, 7), "max_look is Chebyshev: 8 steps of a diagonal");
  CHECK(g.asked == 0, "a pair beyond the look asks for no cell: %d", g.asked);
  CHECK(clear(g, 0, 0, 0, 8, 8) && clear(g, 8, 8, 0, 3, 8), "open ground");
  // one cell beside a diagonal step closes it (the route's rule), whichever side
  set(1, 0, 1);
  CHECK(!clear(g, 0, 0, 1, 1, 4) && !clear(g, 1, 1, 0, 0, 4) && !clear(g, 0, 0, 3, 3, 4), "a cell on one side of a diagonal step");
  CHECK(clear(g, 0, 0, 0, 1, 4) && clear(g, 0, 1, 1, 1, 4) && clear(g, 0, 1, 3, 1, 4), "axis moves beside it");
  set(1, 0, 0); set(0, 1, 1);
  CHECK(!clear(g, 0, 0, 1, 1, 4) && !clear(g, 1, 1, 0, 0, 4), "the other side");
  set(0, 1, 0);
  // the ends and the interior
  set(4, 4, 2);
  CHECK(!clear(g, 4, 4, 4, 4, 1) && !clear(g, 4, 4, 4, 5, 1) && !clear(g, 4, 3, 4, 4, 1) && !clear(g, 4, 2, 4, 6, 8), "V, T and an interior cell SOLID");
  CHECK(clear(g, 4, 3, 3, 3, 1) && clear(g, 5, 2, 5, 6, 8), "beside it");
  CHECK(!clear(g, 3, 3, 5, 5, 8) && !clear(g, 3, 4, 4, 5, 8) && !clear(g, 3, 3, 4, 5, 2), "through it and past its corner");
  set(4, 4, 0);
  // the line is not symmetric.  (0,0) -> (4,2) is (1,1) (2,1) (3,2) (4,2): its first step, a tie rounded away from V, passes between
  // (1,0) and (0,1).  (4,2) -> (0,0) is (3,1) (2,1) (1,0) (0,0): it touches neither (0,1) nor (2,2), but passes between (1,1) and (2,0).
  set(0, 1, 1);
  CHECK(!clear(g, 0, 0, 4, 2, 8) && clear(g, 4, 2, 0, 0, 8), "(0,1) is beside the line from (0,0) only");
  set(0, 1, 0); set(2, 0, 1);
  CHECK(clear(g, 0, 0, 4, 2, 8) && !clear(g, 4, 2, 0, 0, 8), "(2,0) is beside the line from (4,2) only");
  set(2, 0, 0);
  // rule 1 over the two arrays
  const uint8_t blocked[6] = {0, 1, 0, 0, 0, 255};
  const uint32_t dist2[6] = {1, 0, 1, 4, 0xFFFFFFFFu, 9};
  const WaySolid with{blocked, dist2, 4u, 3}, without{blocked, nullptr, 4u, 3}, off{blocked, dist2, 0u, 3};
  CHECK(with(0, 0) && with(0, 1) && with(0, 2) && !with(1, 0) && !with(1, 1) && with(1, 2), "SOLID with a dist2: < min_dist2, NONE is far");
  CHECK(!without(0, 0) && without(0, 1) && !without(0, 2) && !without(1, 0) && without(1, 2), "SOLID without a dist2");
  CHECK(!off(0, 0) && off(0, 1) && !off(1, 1) && off(1, 2), "min_dist2 0 switches the clause off");
}

static void defaults() {
  CHECK(WAY_MAX_LOOK < WAY_THREADS, "one candidate per thread");
  svo_grid_route_params r;
  r.na = 100; r.nb = 300; r.near_r2 = 0; r.near_weight = 0; r.max_cost = 1; r.max_rounds = 1; r.max_path = 777; r.resume = 0;
  svo_grid_clearance_params c;
  c.na = 5; c.nb = 6; c.source_mask = 4; c.max_dist = 64; c.cell_size = 0.375; c.inflate_radius = 0.0;
  P p;
  memset(&p, 0xEE, sizeof p);
  CHECK(way_default_params(&r, &c, &p) == SVO_OK, "the defaults");
  CHECK(p.na == 100 && p.nb == 300 && p.path_stride == 777 && p.max_look == 64 && p.min_dist2 == 0u && p.max_way == 256 && p.cell_size == 0.375, "the defaults' values");
  const char* err = nullptr;
  CHECK(way_params_check(&p, &err) == SVO_OK, "the defaults pass their own check");
  CHECK(way_default_params(nullptr, &c, &p) == SVO_ERR_INVALID && way_default_params(&r, nullptr, &p) == SVO_ERR_INVALID &&
        way_default_params(&r, &c, nullptr) == SVO_ERR_INVALID, "null pointers");
  r.na = 0;
  CHECK(way_default_params(&r, &c, &p) == SVO_ERR_INVALID, "a refused shape");
  r.na = 8192; r.nb = 2049;
  CHECK(way_default_params(&r, &c, &p) == SVO_ERR_INVALID, "a refused area");
  r.na = 100; r.nb = 300; r.max_path = 0;
  CHECK(way_default_params(&r, &c, &p) == SVO_ERR_INVALID, "a refused max_path");
  r.max_path = 1 << 20;
  CHECK(way_default_params(&r, &c, &p) == SVO_OK && p.path_stride == 1 << 20, "max_path 2^20");
  c.cell_size = NAN;
  CHECK(way_default_params(&r, &c, &p) == SVO_ERR_INVALID, "a cell_size that is no number");
}

int main() {
  params();
  pointers();
  lines();
  corners();
  defaults();
  if (fails) { fprintf(stderr, "%d failures\n", fails); return 1; }
  printf("grid waypoints args ok\n");
  return 0;
}
