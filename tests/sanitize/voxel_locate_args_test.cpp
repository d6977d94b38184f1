// host/voxel_locate.h walked on a CPU under ASan + UBSan (tests/test_voxel_locate.py builds and runs it): every refusal at its
// boundary with code, message and order; the sizes; the candidates of 10,000 random poses; the ranking and the selection on
// constructed bests; the loop's three statuses over stub functors; and the candidate matrices the Python restatement gave, bit for
// bit (argv: per pose 7 + 5 * 12 doubles as hexadecimal u64 words, for n_turn 2, turn_step 0.25, up_axis 2).
#include <stdio.h>
#include <stdlib.h>

#include <limits>
#include <random>

#include "voxel_locate.h"

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { ++fails; fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

static void expect(int rc, const char* err, const char* want, const char* where) {
  if (want) CHECK(rc == SVO_ERR_INVALID && err && strcmp(err, want) == 0, "%s: rc %d, message '%s', wanted '%s'", where, rc, err ? err : "(none)", want);
  else CHECK(rc == SVO_OK && err == nullptr, "%s: rc %d, message '%s', wanted acceptance", where, rc, err ? err : "(none)");
}

static const float NaNf = std::numeric_limits<float>::quiet_NaN(), Inff = std::numeric_limits<float>::infinity();
static const svo_voxel_locate_params GOOD = {1, 1, 4, 0.04f, {8, 4, 8}, {512, 128, 512}, 3, 64};
static const svo_voxel_align_params ALIGN = {1, 1, 0.2f, 10, 64, 0.001f, 1e-5f};

template <typename F>
static void param(F set, const char* want, const char* where) {
  svo_voxel_locate_params p = GOOD;
  set(p);
  const char* err = nullptr;
  const int checked = voxel_locate_params_check(&p, &err);
  expect(checked, err, want, where);
  size_t bytes = 7;
  const int rc = voxel_locate_workspace_bytes(&p, &bytes);
  CHECK(want ? (rc == SVO_ERR_INVALID && bytes == 0) : (rc == SVO_OK && bytes == voxel_locate_layout(&p).total && bytes % 256 == 0), "%s: workspace bytes", where);
}

static void params() {
  const char* err = nullptr;
  const int null_rc = voxel_locate_params_check(nullptr, &err);
  expect(null_rc, err, "voxel_map_locate: null params", "null");
  param([](svo_voxel_locate_params&) {}, nullptr, "defaults");
  param([](svo_voxel_locate_params& p) { p.min_count = 0; }, "voxel_map_locate: min_count must be at least 1", "min_count 0");
  param([](svo_voxel_locate_params& p) { p.min_count = 1 << 24; }, nullptr, "min_count 2^24");
  param([](svo_voxel_locate_params& p) { p.up_axis = -1; }, "voxel_map_locate: up_axis outside 0..2", "up_axis -1");
  param([](svo_voxel_locate_params& p) { p.up_axis = 3; }, "voxel_map_locate: up_axis outside 0..2", "up_axis 3");
  param([](svo_voxel_locate_params& p) { p.up_axis = 0; }, nullptr, "up_axis 0");
  param([](svo_voxel_locate_params& p) { p.up_axis = 2; }, nullptr, "up_axis 2");
  param([](svo_voxel_locate_params& p) { p.n_turn = -1; }, "voxel_map_locate: n_turn outside 0..31", "n_turn -1");
  param([](svo_voxel_locate_params& p) { p.n_turn = 32; }, "voxel_map_locate: n_turn outside 0..31", "n_turn 32");
  param([](svo_voxel_locate_params& p) { p.n_turn = 0; }, nullptr, "n_turn 0");
  param([](svo_voxel_locate_params& p) { p.n_turn = 31; }, nullptr, "n_turn 31");
  const char* ts = "voxel_map_locate: turn_step must be finite and in (0, 0.25]";
  for (float bad : {0.0f, -0.04f, nextafterf(0.25f, 1.0f), NaNf, Inff}) param([bad](svo_voxel_locate_params& p) { p.turn_step = bad; }, ts, "turn_step");
  for (float ok : {0.25f, FLT_MIN}) param([ok](svo_voxel_locate_params& p) { p.turn_step = ok; }, nullptr, "turn_step");
  for (int r = 0; r < 3; ++r) {
    param([r](svo_voxel_locate_params& p) { p.box[r] = -1; }, "voxel_map_locate: box outside 0..16", "box -1");
    param([r](svo_voxel_locate_params& p) { p.box[r] = 17; }, "voxel_map_locate: box outside 0..16", "box 17");
    param([r](svo_voxel_locate_params& p) { p.box[r] = 0; }, nullptr, "box 0");
    param([r](svo_voxel_locate_params& p) { p.box[r] = 16; }, nullptr, "box 16");
    param([r](svo_voxel_locate_params& p) { p.dims[r] = 0; }, "voxel_map_occupancy: dims outside 1..2048", "dims 0");
    param([r](svo_voxel_locate_params& p) { p.dims[r] = 2049; }, "voxel_map_occupancy: dims outside 1..2048", "dims 2049");
  }
  param([](svo_voxel_locate_params& p) { p.dims[0] = 96; }, "voxel_map_occupancy: dims[0] must be a multiple of 64", "dims[0] 96");
  param([](svo_voxel_locate_params& p) { p.dims[0] = 64; p.dims[1] = 1; p.dims[2] = 1; }, nullptr, "dims 64 1 1");
  param([](svo_voxel_locate_params& p) { p.dims[0] = 1024; p.dims[1] = 1024; p.dims[2] = 1024; }, nullptr, "dims 2^30");
  param([](svo_voxel_locate_params& p) { p.dims[0] = 2048; p.dims[1] = 1024; p.dims[2] = 1024; }, "voxel_map_occupancy: dims[0] * dims[1] * dims[2] beyond 2^30", "dims 2^31");
  param([](svo_voxel_locate_params& p) { p.dims[0] = 2048; p.dims[1] = 2048; p.dims[2] = 2048; }, "voxel_map_occupancy: dims[0] * dims[1] * dims[2] beyond 2^30", "dims 2^33");
  param([](svo_voxel_locate_params& p) { p.n_refine = 0; }, "voxel_map_locate: n_refine outside 1..63", "n_refine 0");
  param([](svo_voxel_locate_params& p) { p.n_refine = 64; }, "voxel_map_locate: n_refine outside 1..63", "n_refine 64");
  param([](svo_voxel_locate_params& p) { p.n_refine = 63; }, nullptr, "n_refine 63");
  param([](svo_voxel_locate_params& p) { p.min_hits = 0; }, "voxel_map_locate: min_hits must be at least 1", "min_hits 0");
  // the order: the first bad field is the one named
  param([](svo_voxel_locate_params& p) { p.min_hits = 0; p.up_axis = 3; }, "voxel_map_locate: up_axis outside 0..2", "order");
  param([](svo_voxel_locate_params& p) { p.n_refine = 0; p.box[2] = 17; }, "voxel_map_locate: box outside 0..16", "order");
  svo_voxel_locate_params d;
  CHECK(voxel_locate_default_params(0.1f, &d) == SVO_OK && memcmp(&d, &GOOD, sizeof(d)) == 0, "defaults");
  for (float bad : {0.0f, -1.0f, NaNf, Inff}) CHECK(voxel_locate_default_params(bad, &d) == SVO_ERR_INVALID, "defaults refuse %g", (double)bad);
  CHECK(voxel_locate_default_params(0.1f, nullptr) == SVO_ERR_INVALID, "defaults refuse null");
  const VoxelLocateLayout l = voxel_locate_layout(&GOOD);
  CHECK(l.bits == 0 && l.counts == (4u << 20) && l.hits == l.counts + 256 && l.best == l.hits + 93696 && l.total == l.best + 512, "the default layout");
  size_t bytes = 7;
  const int d3[3] = {512, 128, 512};
  CHECK(voxel_occupancy_bytes(d3, &bytes) == SVO_OK && bytes == (4u << 20), "occupancy bytes");
  CHECK(voxel_occupancy_bytes(nullptr, &bytes) == SVO_ERR_INVALID && bytes == 0 && voxel_occupancy_bytes(d3, nullptr) == SVO_ERR_INVALID, "occupancy bytes refusals");
}

static void entries() {
  alignas(256) static unsigned char buf[512];
  const int o[3] = {0, 0, 0}, d[3] = {64, 1, 1}, b[3] = {1, 1, 1};
  const double m[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  const char* err = nullptr;
#define OCC(want, ...) do { err = nullptr; const int rc_ = voxel_occupancy_check(__VA_ARGS__, &err); expect(rc_, err, want, #__VA_ARGS__); } while (0)
  OCC(nullptr, 1, o, d, buf, buf, true);
  OCC("voxel_map_occupancy: min_count must be at least 1", 0, nullptr, d, buf, buf, true);
  OCC("voxel_map_occupancy: null origin", 1, nullptr, nullptr, buf, buf, true);
  for (int r = 0; r < 3; ++r) {
    int lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    lo[r] = -(1 << 20); hi[r] = (1 << 20) - 1;
    OCC(nullptr, 1, lo, d, buf, buf, true);
    OCC(nullptr, 1, hi, d, buf, buf, true);
    lo[r] -= 1; hi[r] += 1;
    OCC("voxel_map_occupancy: origin outside [-2^20, 2^20)", 1, lo, nullptr, buf, buf, true);
    OCC("voxel_map_occupancy: origin outside [-2^20, 2^20)", 1, hi, d, buf, buf, true);
  }
  OCC("voxel_map_occupancy: null dims", 1, o, nullptr, nullptr, buf, true);
  OCC("voxel_map_occupancy: null bits", 1, o, d, nullptr, nullptr, true);
  OCC("voxel_map_occupancy: bits must be 8-byte aligned", 1, o, d, buf + 4, nullptr, true);
  OCC("voxel_map_occupancy: null counts", 1, o, d, buf, nullptr, true);
  OCC("voxel_map_occupancy: counts must be 4-byte aligned", 1, o, d, buf, buf + 2, true);
  OCC(nullptr, 1, o, d, buf + 1, nullptr, false);  // the host form: any alignment, counts optional
  OCC("voxel_map_occupancy: null bits", 1, o, d, nullptr, nullptr, false);
#define SC(want, ...) do { err = nullptr; const int rc_ = voxel_locate_scores_check(__VA_ARGS__, &err); expect(rc_, err, want, #__VA_ARGS__); } while (0)
  SC(nullptr, buf, o, d, buf, 5, m, 1, b, buf, buf);
  SC(nullptr, buf, o, d, nullptr, 0, m, 63, b, buf, buf);
  SC(nullptr, buf, o, d, buf, 1 << 20, m, 1, b, buf, buf);
  SC("voxel_map_locate: n must not be negative", buf, o, d, buf, -1, nullptr, 1, b, buf, buf);
  SC("voxel_map_locate: n beyond 2^20", buf, o, d, buf, (1 << 20) + 1, nullptr, 1, b, buf, buf);
  SC("voxel_map_locate: null mats", buf, o, d, buf, 5, nullptr, 0, b, buf, buf);
  SC("voxel_map_locate: K outside 1..63", buf, o, d, buf, 5, m, 0, nullptr, buf, buf);
  SC("voxel_map_locate: K outside 1..63", buf, o, d, buf, 5, m, 64, b, buf, buf);
  SC("voxel_map_locate: null box", buf, nullptr, d, buf, 5, m, 1, nullptr, buf, buf);
  const int b17[3] = {0, 17, 0}, bm[3] = {0, 0, -1}, b16[3] = {16, 16, 16}, b0[3] = {0, 0, 0};
  SC("voxel_map_locate: box outside 0..16", buf, nullptr, d, buf, 5, m, 1, b17, buf, buf);
  SC("voxel_map_locate: box outside 0..16", buf, o, d, buf, 5, m, 1, bm, buf, buf);
  SC(nullptr, buf, o, d, buf, 5, m, 1, b16, buf, buf);
  SC(nullptr, buf, o, d, buf, 5, m, 1, b0, buf, buf);
  SC("voxel_map_occupancy: null origin", buf, nullptr, nullptr, buf, 5, m, 1, b, buf, buf);
  SC("voxel_map_occupancy: null dims", nullptr, o, nullptr, buf, 5, m, 1, b, buf, buf);
  SC("voxel_map_occupancy: null bits", nullptr, o, d, buf, 5, m, 1, b, nullptr, buf);
  SC("voxel_map_occupancy: bits must be 8-byte aligned", buf + 4, o, d, buf, 5, m, 1, b, nullptr, buf);
  SC("voxel_map_locate: null hits", buf, o, d, buf, 5, m, 1, b, nullptr, nullptr);
  SC("voxel_map_locate: hits must be 4-byte aligned", buf, o, d, buf, 5, m, 1, b, buf + 2, nullptr);
  SC("voxel_map_locate: null best", buf, o, d, nullptr, 5, m, 1, b, buf, nullptr);
  SC("voxel_map_locate: best must be 8-byte aligned", buf, o, d, nullptr, 5, m, 1, b, buf, buf + 4);
  SC("voxel_map_locate: null points", buf, o, d, nullptr, 5, m, 1, b, buf, buf);
  SC("voxel_map_locate: points must be 4-byte aligned", buf, o, d, buf + 2, 5, m, 1, b, buf, buf);
  double q[7] = {1, 0, 0, 0, 0, 0, 0};
  svo_voxel_locate_result res;
#define LOOP(want, ...) do { err = nullptr; const int rc_ = voxel_locate_loop_check(__VA_ARGS__, &err); expect(rc_, err, want, #__VA_ARGS__); } while (0)
  LOOP(nullptr, nullptr, buf, 5, q, &GOOD, &ALIGN, buf, q, &res);
  LOOP(nullptr, buf + 16, nullptr, 0, q, &GOOD, &ALIGN, buf + 256, q, &res);
  LOOP("voxel_map_locate: n must not be negative", nullptr, buf, -1, nullptr, &GOOD, &ALIGN, buf, q, &res);
  LOOP("voxel_map_locate: n beyond 2^20", nullptr, buf, (1 << 20) + 1, nullptr, &GOOD, &ALIGN, buf, q, &res);
  LOOP("voxel_map_locate: null pose7_in", nullptr, buf, 5, nullptr, &GOOD, &ALIGN, buf, nullptr, &res);
  LOOP("voxel_map_locate: null pose7_out", nullptr, buf, 5, q, &GOOD, &ALIGN, buf, nullptr, nullptr);
  LOOP("voxel_map_locate: null result", nullptr, buf, 5, q, nullptr, &ALIGN, buf, q, nullptr);
  LOOP("voxel_map_locate: null params", nullptr, buf, 5, q, nullptr, nullptr, buf, q, &res);
  svo_voxel_locate_params bad = GOOD;
  bad.min_hits = 0;
  LOOP("voxel_map_locate: min_hits must be at least 1", nullptr, buf, 5, q, &bad, nullptr, buf, q, &res);
  LOOP("voxel_map_align: null params", nullptr, buf, 5, q, &GOOD, nullptr, nullptr, q, &res);
  svo_voxel_align_params abad = ALIGN;
  abad.reach = 2;
  LOOP("voxel_map_align: reach outside 0..1", nullptr, buf, 5, q, &GOOD, &abad, nullptr, q, &res);
  LOOP("voxel_map_locate: null workspace", buf + 8, buf, 5, q, &GOOD, &ALIGN, nullptr, q, &res);
  LOOP("voxel_map_locate: workspace must be 256-byte aligned", buf + 8, buf, 5, q, &GOOD, &ALIGN, buf + 128, q, &res);
  LOOP("voxel_map_locate: normals must be 16-byte aligned", buf + 8, nullptr, 5, q, &GOOD, &ALIGN, buf, q, &res);
  LOOP("voxel_map_locate: null points", nullptr, nullptr, 5, q, &GOOD, &ALIGN, buf, q, &res);
  LOOP("voxel_map_locate: points must be 4-byte aligned", nullptr, buf + 1, 5, q, &GOOD, &ALIGN, buf, q, &res);
}

static void origin_is(const double* T, float vs, const int* dims, int* o, const char* want, const char* where) {
  const char* err = nullptr;
  const int rc = voxel_locate_origin(T, vs, dims, o, &err);
  expect(rc, err, want, where);
}

static void origins() {
  const int dims[3] = {512, 128, 512};
  int o[3];
  const double T[3] = {1.234, -0.05, -77.0};
  origin_is(T, 0.1f, dims, o, nullptr, "origin");
  CHECK(o[0] == 12 - 256 && o[1] == -1 - 64 && o[2] == (int)floor(-77.0 / (double)0.1f) - 256, "origin values %d %d %d", o[0], o[1], o[2]);
  // the volume may end exactly where the key range does, on either side (voxel size 1: T is the index)
  const double lo[3] = {-1048576.0 + 256.0, 0.0, 0.0}, hi[3] = {1048576.0 - 256.0, 0.0, 0.0};
  origin_is(lo, 1.0f, dims, o, nullptr, "low end");
  CHECK(o[0] == -(1 << 20), "low end origin");
  origin_is(hi, 1.0f, dims, o, nullptr, "high end");
  CHECK(o[0] + 512 == 1 << 20, "high end origin");
  const char* leaves = "voxel_map_locate: the volume around the prior leaves the key range";
  const char* outside = "voxel_map_locate: the prior's position is outside the key range";
  const double lo1[3] = {-1048576.0 + 255.0, 0.0, 0.0}, hi1[3] = {0.0, 0.0, 1048576.0 - 255.0};
  origin_is(lo1, 1.0f, dims, o, leaves, "below the low end");
  origin_is(hi1, 1.0f, dims, o, leaves, "above the high end");
  for (double bad : {3.0e6, -3.0e6, 1e300, -1e300, (double)NaNf, (double)Inff, -(double)Inff}) {
    const double Tb[3] = {0.0, bad, 0.0};
    origin_is(Tb, 1.0f, dims, o, outside, "far");
  }
}

static void candidates() {
  std::mt19937_64 rng(7);
  std::uniform_real_distribution<double> U(-1.0, 1.0);
  double worst = 0.0;
  for (int it = 0; it < 10000; ++it) {
    double pose[7], u[4], T[3];
    for (int i = 0; i < 4; ++i) pose[i] = U(rng) * (it % 3 == 0 ? 100.0 : 1.0);  // non-unit quaternions too
    for (int i = 4; i < 7; ++i) pose[i] = 50.0 * U(rng);
    voxel_align_from_pose7(pose, u, T);
    svo_voxel_locate_params p = GOOD;
    p.up_axis = it % 3; p.n_turn = 31; p.turn_step = it % 2 ? 0.25f : 0.04f;
    for (int k = 0; k < 63; k += (it % 7) + 1) {
      double uk[4], m[12];
      voxel_locate_candidate(u, T, &p, k, uk, m);
      const double n2 = uk[0] * uk[0] + uk[1] * uk[1] + uk[2] * uk[2] + uk[3] * uk[3], dev = fabs(sqrt(n2) - 1.0);
      worst = dev > worst ? dev : worst;
      for (int r = 0; r < 3; ++r) CHECK(m[4 * r + 3] == T[r], "the candidate keeps T");
      if (k == 31) {
        double R[9], m0[12];
        voxel_align_matrix(u, T, R, m0);
        for (int i = 0; i < 12; ++i) CHECK(fabs(m[i] - m0[i]) <= 1e-15, "b = 0 is no turn: %g vs %g", m[i], m0[i]);
      }
      // the turn is about the world axis: the axis' row of R(u_k) is that of R(u)
      double R0[9], Rk[9];
      voxel_quat_to_R(u, R0);
      voxel_quat_to_R(uk, Rk);
      for (int c = 0; c < 3; ++c) CHECK(fabs(Rk[3 * p.up_axis + c] - R0[3 * p.up_axis + c]) <= 2e-15, "the world axis' row moves: %g", Rk[3 * p.up_axis + c] - R0[3 * p.up_axis + c]);
    }
  }
  CHECK(worst <= 2.2204460492503131e-16, "| |u_k| - 1 | reaches %g: above one ulp (DESIGN 7q)", worst);
  printf("candidates: worst | |u_k| - 1 | = %g\n", worst);
}

static svo_voxel_locate_best B(unsigned hits, int s0 = 0, int s1 = 0, int s2 = 0) { return {hits, s0, s1, s2, 0, 0, 0, 0}; }

static void ranking() {
  const svo_voxel_locate_best best[7] = {B(5), B(90), B(64), B(90), B(63), B(1000), B(64)};
  int order[7];
  CHECK(voxel_locate_rank(best, 7, 64, order) == 5 && order[0] == 5 && order[1] == 1 && order[2] == 3 && order[3] == 2 && order[4] == 6, "rank: ties by ascending k");
  CHECK(voxel_locate_rank(best, 7, 1001, order) == 0, "rank: none left");
  CHECK(voxel_locate_rank(best, 7, 1, order) == 7 && order[5] == 4 && order[6] == 0, "rank: all");
  svo_voxel_locate_best many[63];
  for (int k = 0; k < 63; ++k) many[k] = B((unsigned)(k * 37 % 11));
  int o63[63];
  const int m = voxel_locate_rank(many, 63, 1, o63);
  for (int i = 1; i < m; ++i) {
    const svo_voxel_locate_best &a = many[o63[i - 1]], &b = many[o63[i]];
    CHECK(a.hits_max > b.hits_max || (a.hits_max == b.hits_max && o63[i - 1] < o63[i]), "rank of 63 at %d", i);
  }
  CHECK(m == 63 - 6, "rank of 63: the zeros are dropped (%d)", m);
}

struct Stub {  // per candidate k: the align's verdict
  int status;
  int64_t matched, cost;
};

static void run_loop(const svo_voxel_locate_best* best, const Stub* stub, int n_refine, int want_status, int want_k, int want_rank, int want_refined) {
  svo_voxel_locate_params p = GOOD;
  p.n_turn = 2; p.n_refine = n_refine;
  const double in[7] = {0.9, 0.1, -0.2, 0.05, 1.0, 2.0, 3.0};
  double out[7], coarse_of[5][7];
  svo_voxel_locate_result res;
  const char* err = nullptr;
  int refined = 0, which[5];
  const int rc = voxel_locate_loop(
      in, &p, 0.1f,
      [&](const double*, int K, const int*, svo_voxel_locate_best* b) { CHECK(K == 5, "K"); memcpy(b, best, sizeof(*b) * 5); return (int)SVO_OK; },
      [&](const double* pose, double* o, svo_voxel_align_result* r) {
        // which candidate is this?  the stub's verdicts are told apart by the refinement's number, in rank order
        int order[5];
        const int m = voxel_locate_rank(best, 5, p.min_hits, order);
        CHECK(refined < m, "more refinements than candidates");
        const int k = order[refined];
        which[refined] = k;
        memcpy(coarse_of[refined], pose, sizeof(double) * 7);
        memset(r, 0, sizeof(*r));
        r->status = stub[k].status; r->last_matched = stub[k].matched; r->last_cost = stub[k].cost; r->iterations = k + 1;
        for (int i = 0; i < 7; ++i) o[i] = pose[i] + 1000.0 * (k + 1);
        ++refined;
        return (int)SVO_OK;
      },
      out, &res, &err);
  CHECK(rc == SVO_OK && err == nullptr, "loop rc %d", rc);
  CHECK(res.status == want_status && res.k == want_k && res.rank == want_rank && res.n_refined == want_refined && refined == want_refined,
        "loop: status %d k %d rank %d refined %d (%d), wanted %d %d %d %d", res.status, res.k, res.rank, res.n_refined, refined, want_status, want_k, want_rank, want_refined);
  if (want_status == SVO_VOXEL_LOCATE_NO_CANDIDATE) {
    CHECK(memcmp(out, in, sizeof(in)) == 0 && memcmp(res.coarse_pose7, in, sizeof(in)) == 0 && res.hits == 0 && res.align.iterations == 0, "no candidate: the pose stays");
    return;
  }
  CHECK(res.hits == best[want_k].hits_max && res.shift[0] == best[want_k].s0 && res.shift[1] == best[want_k].s1 && res.shift[2] == best[want_k].s2, "the chosen peak");
  CHECK(memcmp(res.coarse_pose7, coarse_of[want_rank], sizeof(in)) == 0 && which[want_rank] == want_k && res.align.iterations == want_k + 1, "the chosen coarse pose");
  for (int i = 0; i < 7; ++i) CHECK(out[i] == (want_status == SVO_VOXEL_LOCATE_FOUND ? coarse_of[want_rank][i] + 1000.0 * (want_k + 1) : coarse_of[0][i]), "pose7_out[%d]", i);
  // the coarse pose is (u_k, T + s * voxel_size) through step g
  double u[4], T[3], uk[4], m12[12], want[7];
  voxel_align_from_pose7(in, u, T);
  voxel_locate_candidate(u, T, &p, want_k, uk, m12);
  const int s[3] = {best[want_k].s0, best[want_k].s1, best[want_k].s2};
  for (int r = 0; r < 3; ++r) T[r] = T[r] + (double)s[r] * (double)0.1f;
  voxel_align_to_pose7(uk, T, want);
  CHECK(memcmp(want, res.coarse_pose7, sizeof(want)) == 0, "the coarse pose's bits");
}

static void selection() {
  const int C = SVO_VOXEL_ALIGN_CONVERGED, M = SVO_VOXEL_ALIGN_MAX_ITERS, F = SVO_VOXEL_ALIGN_TOO_FEW, D = SVO_VOXEL_ALIGN_DEGENERATE;
  const svo_voxel_locate_best best[5] = {B(70, 1, 2, 3), B(500, -8, 4, 8), B(500, 0, -1, 0), B(63, 5, 5, 5), B(900, -3, 0, 2)};  // ranks: 4, 1, 2, 0
  const Stub most[5] = {{C, 999, 1}, {M, 400, 7}, {C, 450, 9}, {C, 9999, 0}, {C, 300, 5}};
  run_loop(best, most, 3, SVO_VOXEL_LOCATE_FOUND, 2, 2, 3);   // the largest last_matched among the first three ranks
  run_loop(best, most, 4, SVO_VOXEL_LOCATE_FOUND, 0, 3, 4);   // a fourth refinement reaches k = 0
  run_loop(best, most, 63, SVO_VOXEL_LOCATE_FOUND, 0, 3, 4);  // n_refine beyond the candidates
  run_loop(best, most, 1, SVO_VOXEL_LOCATE_FOUND, 4, 0, 1);
  const Stub ties[5] = {{C, 400, 3}, {C, 400, 7}, {M, 400, 7}, {C, 0, 0}, {C, 400, 8}};
  run_loop(best, ties, 3, SVO_VOXEL_LOCATE_FOUND, 1, 1, 3);  // equal matches: the smaller cost; equal cost: the earlier rank
  run_loop(best, ties, 4, SVO_VOXEL_LOCATE_FOUND, 0, 3, 4);
  const Stub some[5] = {{C, 5, 5}, {F, 9000, 0}, {M, 10, 10}, {C, 0, 0}, {D, 9000, 0}};
  run_loop(best, some, 3, SVO_VOXEL_LOCATE_FOUND, 2, 2, 3);  // TOO_FEW and DEGENERATE are not eligible
  const Stub none[5] = {{F, 1, 1}, {D, 2, 2}, {F, 3, 3}, {C, 4, 4}, {D, 5, 5}};
  run_loop(best, none, 3, SVO_VOXEL_LOCATE_UNREFINED, 4, 0, 3);
  const svo_voxel_locate_best low[5] = {B(63), B(0), B(10), B(63), B(1)};
  run_loop(low, most, 3, SVO_VOXEL_LOCATE_NO_CANDIDATE, -1, -1, 0);
  // an error of a functor ends the loop and nothing is written
  svo_voxel_locate_params p = GOOD;
  const double in[7] = {1, 0, 0, 0, 0, 0, 0};
  double out[7] = {7, 7, 7, 7, 7, 7, 7};
  svo_voxel_locate_result res;
  memset(&res, 0x5A, sizeof(res));
  const char* err = nullptr;
  int rc = voxel_locate_loop(in, &p, 0.1f, [&](const double*, int, const int*, svo_voxel_locate_best*) { return -5; },
                             [&](const double*, double*, svo_voxel_align_result*) { return 0; }, out, &res, &err);
  CHECK(rc == -5 && out[0] == 7 && res.status == 0x5A5A5A5A, "an error of the scores");
  rc = voxel_locate_loop(in, &p, 0.1f, [&](const double*, int, const int*, svo_voxel_locate_best* b) { memcpy(b, best, sizeof(*b) * 5); for (int k = 5; k < 9; ++k) b[k] = B(0); return 0; },
                         [&](const double*, double*, svo_voxel_align_result*) { return -6; }, out, &res, &err);
  CHECK(rc == -6 && out[0] == 7 && res.status == 0x5A5A5A5A, "an error of the refinement");
  const double far[7] = {1, 0, 0, 0, 2.0e5, 0, 0};
  rc = voxel_locate_loop(far, &p, 0.1f, [&](const double*, int, const int*, svo_voxel_locate_best*) { CHECK(false, "scores after a refusal"); return 0; },
                         [&](const double*, double*, svo_voxel_align_result*) { return 0; }, out, &res, &err);
  CHECK(rc == SVO_ERR_INVALID && err && strstr(err, "leaves the key range") && out[0] == 7, "the origin's refusal");
}

static double from_hex(const char* s) {
  const unsigned long long w = strtoull(s, nullptr, 16);
  double d;
  memcpy(&d, &w, sizeof(d));
  return d;
}

static void against_python(int argc, char** argv) {
  CHECK((argc - 1) % 67 == 0 && argc > 1, "argv: %d words", argc - 1);
  svo_voxel_locate_params p = GOOD;
  p.n_turn = 2; p.turn_step = 0.25f; p.up_axis = 2;
  for (int at = 1; at + 67 <= argc; at += 67) {
    double pose[7], u[4], T[3];
    for (int i = 0; i < 7; ++i) pose[i] = from_hex(argv[at + i]);
    voxel_align_from_pose7(pose, u, T);
    for (int k = 0; k < 5; ++k) {
      double uk[4], m[12];
      voxel_locate_candidate(u, T, &p, k, uk, m);
      for (int i = 0; i < 12; ++i) {
        const double want = from_hex(argv[at + 7 + 12 * k + i]);
        CHECK(memcmp(&want, &m[i], sizeof(want)) == 0, "candidate %d word %d: %.17g, Python gave %.17g", k, i, m[i], want);
      }
    }
  }
}

int main(int argc, char** argv) {
  params();
  entries();
  origins();
  candidates();
  ranking();
  selection();
  against_python(argc, argv);
  if (fails) { fprintf(stderr, "%d checks failed\n", fails); return 1; }
  printf("voxel locate args ok\n");
  return 0;
}
