// The voxel map align's GPU-free host logic (stereo_vo_amd/host/voxel_align.h) walked on the host, under ASan + UBSan: every refusal
// at its boundary with its code and its exact message and the order of the refusals, the defaults, Q_S at +-0.5/S, at the doubles next
// to them and at the largest magnitudes the contract's bounds allow, the Cholesky solve on a hand-made SPD matrix, on a singular one
// and on one with a NaN, the pose update keeping |u| = 1 to one ulp over 10,000 random steps, the round trips pose7 -> (u, T) ->
// pose7, and the loop over a functor for every status.
#include <limits.h>
#include <stdio.h>
#include <string.h>

#include <limits>
#include <random>

#include "voxel_align.h"

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { ++fails; fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

// rc is the refusal with exactly this message, or (want == nullptr) SVO_OK with the message untouched
static void expect(int rc, const char* err, const char* want, const char* where) {
  if (want) CHECK(rc == SVO_ERR_INVALID && err && strcmp(err, want) == 0, "%s: rc %d, message '%s', wanted '%s'", where, rc, err ? err : "(none)", want);
  else CHECK(rc == SVO_OK && err == nullptr, "%s: rc %d, message '%s', wanted acceptance", where, rc, err ? err : "(none)");
}
#define EXPECT(call, want, where) do { const char* err = nullptr; const int rc_ = (call); expect(rc_, err, want, where); } while (0)

static const double NaN = std::numeric_limits<double>::quiet_NaN(), Inf = std::numeric_limits<double>::infinity();
static const svo_voxel_align_params GOOD = {1, 1, 0.2f, 10, 64, 0.001f, 1e-5f};

static void params() {
  const char* mc = "voxel_map_align: min_count must be at least 1";
  const char* re = "voxel_map_align: reach outside 0..1";
  const char* md = "voxel_map_align: max_dist must be finite and in (0, 8]";
  const char* mi = "voxel_map_align: max_iters must be at least 1";
  const char* mm = "voxel_map_align: min_matches must be at least 6";
  const char* et = "voxel_map_align: eps_t must be finite and not negative";
  const char* er = "voxel_map_align: eps_r must be finite and not negative";
  const struct { svo_voxel_align_params p; const char* want; } cases[] = {
      {GOOD, nullptr},
      {{0, 1, 0.2f, 10, 64, 0.001f, 1e-5f}, mc}, {{-3, 1, 0.2f, 10, 64, 0.001f, 1e-5f}, mc}, {{INT_MAX, 1, 0.2f, 10, 64, 0.001f, 1e-5f}, nullptr},
      {{1, -1, 0.2f, 10, 64, 0.001f, 1e-5f}, re}, {{1, 2, 0.2f, 10, 64, 0.001f, 1e-5f}, re}, {{1, 0, 0.2f, 10, 64, 0.001f, 1e-5f}, nullptr},
      {{1, 1, 0.0f, 10, 64, 0.001f, 1e-5f}, md}, {{1, 1, -0.0f, 10, 64, 0.001f, 1e-5f}, md}, {{1, 1, -1.0f, 10, 64, 0.001f, 1e-5f}, md},
      {{1, 1, FLT_MIN, 10, 64, 0.001f, 1e-5f}, nullptr}, {{1, 1, 8.0f, 10, 64, 0.001f, 1e-5f}, nullptr},
      {{1, 1, nextafterf(8.0f, 9.0f), 10, 64, 0.001f, 1e-5f}, md}, {{1, 1, (float)NaN, 10, 64, 0.001f, 1e-5f}, md},
      {{1, 1, (float)Inf, 10, 64, 0.001f, 1e-5f}, md},
      {{1, 1, 0.2f, 0, 64, 0.001f, 1e-5f}, mi}, {{1, 1, 0.2f, 1, 64, 0.001f, 1e-5f}, nullptr},
      {{1, 1, 0.2f, 10, 5, 0.001f, 1e-5f}, mm}, {{1, 1, 0.2f, 10, 6, 0.001f, 1e-5f}, nullptr},
      {{1, 1, 0.2f, 10, 64, -FLT_MIN, 1e-5f}, et}, {{1, 1, 0.2f, 10, 64, 0.0f, 1e-5f}, nullptr}, {{1, 1, 0.2f, 10, 64, (float)Inf, 1e-5f}, et},
      {{1, 1, 0.2f, 10, 64, (float)NaN, 1e-5f}, et}, {{1, 1, 0.2f, 10, 64, FLT_MAX, 1e-5f}, nullptr},
      {{1, 1, 0.2f, 10, 64, 0.001f, -1.0f}, er}, {{1, 1, 0.2f, 10, 64, 0.001f, 0.0f}, nullptr}, {{1, 1, 0.2f, 10, 64, 0.001f, (float)Inf}, er},
      {{1, 1, 0.2f, 10, 64, 0.001f, (float)NaN}, er},
      // the order: the first bad field is the one named
      {{0, 2, 0.0f, 0, 0, -1.0f, -1.0f}, mc}, {{1, 2, 0.0f, 0, 0, -1.0f, -1.0f}, re}, {{1, 1, 0.0f, 0, 0, -1.0f, -1.0f}, md},
      {{1, 1, 1.0f, 0, 0, -1.0f, -1.0f}, mi}, {{1, 1, 1.0f, 1, 0, -1.0f, -1.0f}, mm}, {{1, 1, 1.0f, 1, 6, -1.0f, -1.0f}, et}};
  for (const auto& c : cases) EXPECT(voxel_align_params_check(&c.p, &err), c.want, "params");
  EXPECT(voxel_align_params_check(nullptr, &err), "voxel_map_align: null params", "null params");
}

static void entries() {
  alignas(16) static unsigned char buf[64];
  const double m[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  const svo_voxel_align_params bad = {0, 1, 0.2f, 10, 64, 0.001f, 1e-5f};
  const char* neg = "voxel_map_align: n must not be negative";
  const char* big = "voxel_map_align: n beyond 2^20";
  EXPECT(voxel_align_sums_check(buf, 5, m, &GOOD, buf + 8, &err), nullptr, "sums ok");
  EXPECT(voxel_align_sums_check(nullptr, 0, m, &GOOD, buf, &err), nullptr, "sums n == 0 with null points");
  EXPECT(voxel_align_sums_check(buf, 1 << 20, m, &GOOD, buf, &err), nullptr, "sums n == 2^20");
  // each refusal with everything behind it bad as well: the order
  EXPECT(voxel_align_sums_check(nullptr, -1, nullptr, nullptr, nullptr, &err), neg, "sums n < 0");
  EXPECT(voxel_align_sums_check(nullptr, INT_MIN, nullptr, nullptr, nullptr, &err), neg, "sums n = INT_MIN");
  EXPECT(voxel_align_sums_check(nullptr, (1 << 20) + 1, nullptr, nullptr, nullptr, &err), big, "sums n > 2^20");
  EXPECT(voxel_align_sums_check(nullptr, INT_MAX, nullptr, nullptr, nullptr, &err), big, "sums n = INT_MAX");
  EXPECT(voxel_align_sums_check(nullptr, 5, nullptr, nullptr, nullptr, &err), "voxel_map_align: null c2w12", "sums null matrix");
  EXPECT(voxel_align_sums_check(nullptr, 5, m, nullptr, nullptr, &err), "voxel_map_align: null params", "sums null params");
  EXPECT(voxel_align_sums_check(nullptr, 5, m, &bad, nullptr, &err), "voxel_map_align: min_count must be at least 1", "sums bad params");
  EXPECT(voxel_align_sums_check(nullptr, 5, m, &GOOD, nullptr, &err), "voxel_map_align: null sums", "sums null sums");
  for (int off = 1; off < 8; ++off)
    EXPECT(voxel_align_sums_check(nullptr, 5, m, &GOOD, buf + off, &err), "voxel_map_align: sums must be 8-byte aligned", "sums alignment");
  EXPECT(voxel_align_sums_check(nullptr, 5, m, &GOOD, buf + 8, &err), "voxel_map_align: null points", "sums null points");
  for (int off = 1; off < 4; ++off)
    EXPECT(voxel_align_sums_check(buf + off, 5, m, &GOOD, buf + 8, &err), "voxel_map_align: points must be 4-byte aligned", "points alignment");
  EXPECT(voxel_align_sums_check(buf + 4, 5, m, &GOOD, buf + 8, &err), nullptr, "points at 4");
  // the loop's entry
  double q[7] = {1, 0, 0, 0, 0, 0, 0}, out[7];
  svo_voxel_align_result res;
  EXPECT(voxel_align_loop_check(buf, 5, q, &GOOD, out, &res, &err), nullptr, "loop ok");
  EXPECT(voxel_align_loop_check(nullptr, 0, q, &GOOD, out, &res, &err), nullptr, "loop n == 0");
  EXPECT(voxel_align_loop_check(nullptr, -1, nullptr, nullptr, nullptr, nullptr, &err), neg, "loop n < 0");
  EXPECT(voxel_align_loop_check(nullptr, (1 << 20) + 1, nullptr, nullptr, nullptr, nullptr, &err), big, "loop n > 2^20");
  EXPECT(voxel_align_loop_check(nullptr, 5, nullptr, nullptr, nullptr, nullptr, &err), "voxel_map_align: null pose7_in", "loop pose7_in");
  EXPECT(voxel_align_loop_check(nullptr, 5, q, nullptr, nullptr, nullptr, &err), "voxel_map_align: null pose7_out", "loop pose7_out");
  EXPECT(voxel_align_loop_check(nullptr, 5, q, nullptr, out, nullptr, &err), "voxel_map_align: null result", "loop result");
  EXPECT(voxel_align_loop_check(nullptr, 5, q, nullptr, out, &res, &err), "voxel_map_align: null params", "loop params");
  EXPECT(voxel_align_loop_check(nullptr, 5, q, &bad, out, &res, &err), "voxel_map_align: min_count must be at least 1", "loop bad params");
  EXPECT(voxel_align_loop_check(nullptr, 5, q, &GOOD, out, &res, &err), "voxel_map_align: null points", "loop points");
  EXPECT(voxel_align_loop_check(buf + 2, 5, q, &GOOD, out, &res, &err), "voxel_map_align: points must be 4-byte aligned", "loop alignment");
}

static void defaults() {
  svo_voxel_align_params p;
  CHECK(voxel_align_default_params(0.1f, &p) == SVO_OK && p.min_count == 1 && p.reach == 1 && p.max_dist == 0.2f && p.max_iters == 10 &&
        p.min_matches == 64 && p.eps_t == 0.1f / 100.0f && p.eps_r == 1e-5f, "defaults at 0.1");
  EXPECT(voxel_align_params_check(&p, &err), nullptr, "the defaults pass");
  CHECK(voxel_align_default_params(4.0f, &p) == SVO_OK && p.max_dist == 8.0f, "defaults at 4");
  CHECK(voxel_align_default_params(100.0f, &p) == SVO_OK && p.max_dist == 8.0f, "defaults at 100: max_dist is capped");
  EXPECT(voxel_align_params_check(&p, &err), nullptr, "the capped defaults pass");
  CHECK(voxel_align_default_params(FLT_MAX, &p) == SVO_OK && p.max_dist == 8.0f, "defaults at FLT_MAX");
  for (float bad : {0.0f, -1.0f, (float)NaN, (float)Inf}) CHECK(voxel_align_default_params(bad, &p) == SVO_ERR_INVALID, "defaults refuse %g", (double)bad);
  CHECK(voxel_align_default_params(0.1f, nullptr) == SVO_ERR_INVALID, "defaults refuse null");
}

static void quantiser() {
  for (const double S : {VOXEL_ALIGN_S16, VOXEL_ALIGN_S28}) {
    const double h = 0.5 / S;  // exact: S is a power of two
    CHECK(voxel_align_q(h, S) == 1, "Q(+0.5/S)");
    CHECK(voxel_align_q(nextafter(h, 0.0), S) == 1, "Q just below +0.5/S");  // (0.5 - 2^-54) + 0.5 rounds to 1.0: the stated operations, not the real numbers
    CHECK(voxel_align_q(0.5 * h, S) == 0, "Q(+0.25/S)");
    CHECK(voxel_align_q(nextafter(h, 1.0), S) == 1, "Q just above +0.5/S");
    CHECK(voxel_align_q(-h, S) == 0, "Q(-0.5/S)");
    CHECK(voxel_align_q(nextafter(-h, 0.0), S) == 0, "Q just above -0.5/S");
    CHECK(voxel_align_q(nextafter(-h, -1.0), S) == -1, "Q just below -0.5/S");
    CHECK(voxel_align_q(0.0, S) == 0 && voxel_align_q(-0.0, S) == 0 && voxel_align_q(1.0, S) == (long long)S && voxel_align_q(-1.0, S) == -(long long)S, "Q at 0 and 1");
    CHECK(voxel_align_q(3.0 * h, S) == 2 && voxel_align_q(-3.0 * h, S) == -1, "Q at +-1.5/S");
  }
  // the largest magnitudes of rule 5, each times the 2^20 records of a launch, without overflow
  const long long n = SVO_VOXEL_ALIGN_MAX_POINTS;
  const double P = nextafter(1024.0, 0.0), c = nextafter(8.0, 9.0);
  const struct { double t, S; long long bound; } big[] = {{P, VOXEL_ALIGN_S16, 1ll << 26}, {P * P, VOXEL_ALIGN_S16, 1ll << 36}, {c, VOXEL_ALIGN_S28, (1ll << 31) + 1},
                                                           {16384.0, VOXEL_ALIGN_S28, 1ll << 42}, {64.0, VOXEL_ALIGN_S28, 1ll << 34}};
  for (const auto& b : big) {
    const long long plus = voxel_align_q(b.t, b.S), minus = voxel_align_q(-b.t, b.S);
    CHECK(plus <= b.bound && minus >= -b.bound && plus > 0 && minus < 0, "Q(%g, %g) = %lld, %lld", b.t, b.S, plus, minus);
    long long sum = 0, neg = 0;
    CHECK(!__builtin_mul_overflow(plus, n, &sum) && !__builtin_mul_overflow(minus, n, &neg) && sum <= (1ll << 62) && neg >= -(1ll << 62), "n terms of %g", b.t);
  }
}

static void fill_spd(double H[6][6], double g[6], std::mt19937_64& rng) {
  std::uniform_real_distribution<double> u(-1.0, 1.0);
  double M[6][6];
  for (auto& row : M) for (double& v : row) v = u(rng);
  for (int i = 0; i < 6; ++i) {
    for (int j = 0; j < 6; ++j) {
      H[i][j] = i == j ? 0.5 : 0.0;
      for (int k = 0; k < 6; ++k) H[i][j] += M[i][k] * M[j][k];
    }
    g[i] = u(rng);
  }
}

static void cholesky() {
  // hand-made: H = L L^T with L = lower(1..), so the solution is known in closed form
  const double L[6][6] = {{2, 0, 0, 0, 0, 0}, {1, 3, 0, 0, 0, 0}, {-1, 2, 1, 0, 0, 0}, {0, 1, -2, 4, 0, 0}, {3, 0, 1, 1, 2, 0}, {1, -1, 0, 2, 1, 5}};
  const double want[6] = {1, -2, 3, -4, 5, -6};
  double H[6][6], g[6], xi[6];
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j) {
      H[i][j] = 0.0;
      for (int k = 0; k < 6; ++k) H[i][j] += L[i][k] * L[j][k];
    }
  for (int i = 0; i < 6; ++i) {
    g[i] = 0.0;
    for (int j = 0; j < 6; ++j) g[i] -= H[i][j] * want[j];
  }
  CHECK(voxel_align_solve(H, g, xi), "hand-made SPD refused");
  for (int i = 0; i < 6; ++i) CHECK(xi[i] == want[i], "hand-made: xi[%d] = %.17g", i, xi[i]);  // small integers: exact
  std::mt19937_64 rng(5);
  for (int t = 0; t < 200; ++t) {
    fill_spd(H, g, rng);
    CHECK(voxel_align_solve(H, g, xi), "random SPD refused");
    for (int i = 0; i < 6; ++i) {
      double r = g[i];
      for (int j = 0; j < 6; ++j) r += H[i][j] * xi[j];
      CHECK(fabs(r) < 1e-9, "random SPD: residual %g", r);
    }
  }
  // singular: a zero row and column at each place; a rank-one matrix; the zero matrix
  for (int z = 0; z < 6; ++z) {
    fill_spd(H, g, rng);
    for (int k = 0; k < 6; ++k) H[z][k] = H[k][z] = 0.0;
    double keep[6] = {7, 7, 7, 7, 7, 7};
    CHECK(!voxel_align_solve(H, g, keep) && keep[0] == 7 && keep[5] == 7, "zero row %d accepted, or xi written", z);
  }
  for (int i = 0; i < 6; ++i) for (int j = 0; j < 6; ++j) H[i][j] = 1.0;
  CHECK(!voxel_align_solve(H, g, xi), "rank one accepted");
  for (auto& row : H) for (double& v : row) v = 0.0;
  CHECK(!voxel_align_solve(H, g, xi), "zero accepted");
  // a NaN or an infinity anywhere the factorisation reads; a negative pivot
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j <= i; ++j)
      for (const double v : {NaN, Inf}) {
        fill_spd(H, g, rng);
        H[i][j] = H[j][i] = v;
        CHECK(!voxel_align_solve(H, g, xi), "%g at (%d, %d) accepted", v, i, j);
      }
  fill_spd(H, g, rng);
  H[3][3] = -1.0;
  CHECK(!voxel_align_solve(H, g, xi), "a negative pivot accepted");
}

static void normal_equations() {
  int64_t w[VOXEL_ALIGN_WORDS] = {0};
  // one point P = (1, 2, 3) with residual c = (0.5, -0.25, 0.125)
  const double P[3] = {1, 2, 3}, c[3] = {0.5, -0.25, 0.125};
  w[0] = 1;
  for (int i = 0; i < 3; ++i) w[1 + i] = voxel_align_q(P[i], VOXEL_ALIGN_S16);
  int k = 4;
  for (int i = 0; i < 3; ++i) for (int j = i; j < 3; ++j) w[k++] = voxel_align_q(P[i] * P[j], VOXEL_ALIGN_S16);
  for (int i = 0; i < 3; ++i) w[10 + i] = voxel_align_q(c[i], VOXEL_ALIGN_S28);
  const double x[3] = {P[1] * c[2] - P[2] * c[1], P[2] * c[0] - P[0] * c[2], P[0] * c[1] - P[1] * c[0]};
  for (int i = 0; i < 3; ++i) w[13 + i] = voxel_align_q(x[i], VOXEL_ALIGN_S28);
  double H[6][6], g[6];
  voxel_align_normal(w, H, g);
  // J = [I | -[P]x]: H = J^T J, g = J^T c
  const double J[3][6] = {{1, 0, 0, 0, P[2], -P[1]}, {0, 1, 0, -P[2], 0, P[0]}, {0, 0, 1, P[1], -P[0], 0}};
  for (int i = 0; i < 6; ++i) {
    double gi = 0.0;
    for (int r = 0; r < 3; ++r) gi += J[r][i] * c[r];
    CHECK(g[i] == gi, "g[%d] = %g, wanted %g", i, g[i], gi);
    for (int j = 0; j < 6; ++j) {
      double h = 0.0;
      for (int r = 0; r < 3; ++r) h += J[r][i] * J[r][j];
      CHECK(H[i][j] == h, "H[%d][%d] = %g, wanted %g", i, j, H[i][j], h);
    }
  }
}

static void poses() {
  std::mt19937_64 rng(11);
  std::uniform_real_distribution<double> u(-1.0, 1.0);
  // round trips: pose7 -> (u, T) -> pose7 gives the normalised quaternion and the same translation; the two matrices agree
  for (int t = 0; t < 1000; ++t) {
    double q[7], uq[4], T[3], back[7], R[9], m12[12], lib[12];
    const double scale = t % 3 == 0 ? 1.0 : (t % 3 == 1 ? 0.37 : 5.0);
    for (double& v : q) v = u(rng) * 4.0;
    const double s = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    voxel_align_from_pose7(q, uq, T);
    voxel_align_to_pose7(uq, T, back);
    for (int i = 0; i < 4; ++i) CHECK(fabs(back[i] - q[i] / s) < 1e-15, "round trip q[%d]: %g against %g", i, back[i], q[i] / s);
    for (int i = 4; i < 7; ++i) CHECK(fabs(back[i] - q[i]) < 1e-13, "round trip t[%d]: %g against %g", i, back[i], q[i]);
    voxel_align_matrix(uq, T, R, m12);
    voxel_pose7_to_cam_to_world(q, lib);
    for (int i = 0; i < 12; ++i) CHECK(fabs(m12[i] - lib[i]) < 1e-13, "matrix[%d]: %g against %g", i, m12[i], lib[i]);
    (void)scale;
  }
  // the update keeps |u| = 1 to one ulp over 10,000 random steps (the norm taken in long double)
  double uq[4] = {1, 0, 0, 0}, T[3] = {0, 0, 0}, R[9], m12[12];
  long double worst = 0.0L;
  for (int t = 0; t < 10000; ++t) {
    double xi[6];
    for (double& v : xi) v = u(rng) * (t % 2 ? 0.3 : 1e-3);
    voxel_align_matrix(uq, T, R, m12);
    voxel_align_update(uq, T, R, xi);
    long double n2 = 0.0L;
    for (const double v : uq) n2 += (long double)v * (long double)v;
    const long double dev = fabsl(sqrtl(n2) - 1.0L);
    worst = dev > worst ? dev : worst;
  }
  CHECK(worst <= (long double)DBL_EPSILON, "|u| drifts: %Lg", worst);
  printf("worst | |u| - 1 | over 10000 steps: %Lg\n", worst);
  // a pure translation step moves T by R v and leaves u alone
  double u0[4] = {0.5, 0.5, 0.5, 0.5}, T0[3] = {1, 2, 3};
  const double xi[6] = {0.25, -0.5, 1.0, 0, 0, 0};
  voxel_align_matrix(u0, T0, R, m12);
  voxel_align_update(u0, T0, R, xi);
  CHECK(u0[0] == 0.5 && u0[1] == 0.5 && u0[2] == 0.5 && u0[3] == 0.5, "translation step turned u");
  CHECK(T0[0] == 1 + 1.0 && T0[1] == 2 + 0.25 && T0[2] == 3 - 0.5, "translation step: T = %g %g %g", T0[0], T0[1], T0[2]);  // R(0.5,0.5,0.5,0.5): x->y->z->x
}

static void the_loop() {
  const double pose[7] = {0.9, 0.1, -0.2, 0.05, 1, 2, 3};
  double out[7];
  svo_voxel_align_result res;
  int calls = 0;
  // too few at once: the input pose comes back bit for bit
  auto few = [&](const double*, int64_t* w) { ++calls; memset(w, 0, sizeof(int64_t) * VOXEL_ALIGN_WORDS); w[17] = 63; w[16] = 5; return (int)SVO_OK; };
  CHECK(voxel_align_loop(pose, &GOOD, few, out, &res) == SVO_OK && res.status == SVO_VOXEL_ALIGN_TOO_FEW && res.iterations == 1 && calls == 1 &&
        memcmp(out, pose, sizeof(out)) == 0 && res.first_matched == 63 && res.last_cost == 5 && res.xi[0] == 0.0, "too few");
  // a functor's error ends the loop and writes nothing
  double keep[7] = {9, 9, 9, 9, 9, 9, 9};
  res.status = 77;
  auto broken = [&](const double*, int64_t*) { return (int)SVO_ERR_HIP; };
  CHECK(voxel_align_loop(pose, &GOOD, broken, keep, &res) == SVO_ERR_HIP && keep[0] == 9 && res.status == 77, "functor error");
  // degenerate: enough matches, all sums zero but N
  auto flat = [&](const double*, int64_t* w) { memset(w, 0, sizeof(int64_t) * VOXEL_ALIGN_WORDS); w[0] = w[17] = 100; return (int)SVO_OK; };
  CHECK(voxel_align_loop(pose, &GOOD, flat, out, &res) == SVO_OK && res.status == SVO_VOXEL_ALIGN_DEGENERATE && memcmp(out, pose, sizeof(out)) == 0, "degenerate");
  // a well-posed cloud (8 corners of a cube) with zero residual: xi = 0, converged after one iteration, the pose normalised
  auto cube = [&](const double*, int64_t* w) {
    memset(w, 0, sizeof(int64_t) * VOXEL_ALIGN_WORDS);
    for (int c = 0; c < 8; ++c) {
      const double P[3] = {c & 1 ? 1.0 : -1.0, c & 2 ? 1.0 : -1.0, c & 4 ? 3.0 : 1.0};
      w[0] += 1; w[17] += 1;
      for (int i = 0; i < 3; ++i) w[1 + i] += voxel_align_q(P[i], VOXEL_ALIGN_S16);
      int k = 4;
      for (int i = 0; i < 3; ++i) for (int j = i; j < 3; ++j) w[k++] += voxel_align_q(P[i] * P[j], VOXEL_ALIGN_S16);
    }
    return (int)SVO_OK;
  };
  svo_voxel_align_params p6 = GOOD;
  p6.min_matches = 6;
  CHECK(voxel_align_loop(pose, &p6, cube, out, &res) == SVO_OK && res.status == SVO_VOXEL_ALIGN_CONVERGED && res.iterations == 1, "cube: status %d", res.status);
  for (int i = 0; i < 6; ++i) CHECK(res.xi[i] == 0.0, "cube: xi[%d] = %g", i, res.xi[i]);
  // a constant pull: never converges, max_iters launches
  calls = 0;
  auto pull = [&](const double* m, int64_t* w) { cube(m, w); ++calls; w[10] = voxel_align_q(0.5, VOXEL_ALIGN_S28) * 8; w[14] = voxel_align_q(0.5 * 16.0, VOXEL_ALIGN_S28); return (int)SVO_OK; };
  CHECK(voxel_align_loop(pose, &p6, pull, out, &res) == SVO_OK && res.status == SVO_VOXEL_ALIGN_MAX_ITERS && res.iterations == 10 && calls == 10, "pull: status %d", res.status);
  CHECK(fabs(res.xi[0] + 0.5) < 1e-12 && fabs(res.xi[1]) < 1e-12 && fabs(res.xi[3]) < 1e-12, "pull: xi = %g %g %g", res.xi[0], res.xi[1], res.xi[3]);
  // in place: pose7_out may be pose7_in
  double io[7];
  memcpy(io, pose, sizeof(io));
  CHECK(voxel_align_loop(io, &p6, pull, io, &res) == SVO_OK && memcmp(io, out, sizeof(io)) == 0, "in place");
}

int main() {
  params();
  entries();
  defaults();
  quantiser();
  cholesky();
  normal_equations();
  poses();
  the_loop();
  if (fails) { fprintf(stderr, "%d failures\n", fails); return 1; }
  printf("voxel align args ok\n");
  return 0;
}
