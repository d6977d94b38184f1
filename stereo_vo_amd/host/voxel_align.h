// The voxel map align's host logic that needs no GPU (include/svo.h, "Voxel map align"): the argument checks with their
// message texts and their order, the defaults, Q_S, the assembly of H and g from the 21 words, the unpivoted Cholesky solve, the
// conversion between pose7 and the camera->world (u, T), the pose update and the whole loop over a functor that supplies the sums
// of one matrix.  A refusal is SVO_ERR_INVALID with *err set to the message; csrc/voxel_align.hip stores it in the context, supplies
// the functor (one launch and one 256-byte copy) and keeps no second copy of anything here.
// tests/sanitize/voxel_align_args_test.cpp walks all of it on a CPU.
#ifndef SVO_VOXEL_ALIGN_H_
#define SVO_VOXEL_ALIGN_H_
#include <float.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "voxel_args.h"

constexpr int VOXEL_ALIGN_WORDS = SVO_VOXEL_ALIGN_WORDS;
constexpr int VOXEL_ALIGN_COUNTS = 17;  // words 17..20: n_matched, n_rejected, n_unmatched, n_far
constexpr double VOXEL_ALIGN_S16 = 65536.0, VOXEL_ALIGN_S28 = 268435456.0;
constexpr double VOXEL_ALIGN_LIMIT = 1048575.0;  // rule 1: one voxel inside the key range
constexpr float VOXEL_ALIGN_MAX_DIST = 8.0f, VOXEL_ALIGN_MAX_ABS = 1024.0f;

// Q_S(t) = (int64)floor(t*S + 0.5): multiply, add, floor, convert (rule 4).
VOXEL_HD inline long long voxel_align_q(double t, double S) { return (long long)floor(t * S + 0.5); }

// ----------------------------------------------------------------------------- the checks, in the contract's order
inline int voxel_align_params_check(const svo_voxel_align_params* p, const char** err) {
  VOXEL_REFUSE(p, "voxel_map_align: null params");
  VOXEL_REFUSE(p->min_count >= 1, "voxel_map_align: min_count must be at least 1");
  VOXEL_REFUSE(p->reach >= 0 && p->reach <= 1, "voxel_map_align: reach outside 0..1");
  VOXEL_REFUSE(p->max_dist > 0.0f && p->max_dist <= VOXEL_ALIGN_MAX_DIST, "voxel_map_align: max_dist must be finite and in (0, 8]");  // a NaN fails the first test
  VOXEL_REFUSE(p->max_iters >= 1, "voxel_map_align: max_iters must be at least 1");
  VOXEL_REFUSE(p->min_matches >= 6, "voxel_map_align: min_matches must be at least 6");
  VOXEL_REFUSE(p->eps_t >= 0.0f && p->eps_t <= FLT_MAX, "voxel_map_align: eps_t must be finite and not negative");
  VOXEL_REFUSE(p->eps_r >= 0.0f && p->eps_r <= FLT_MAX, "voxel_map_align: eps_r must be finite and not negative");
  return SVO_OK;
}

inline int voxel_align_n_check(int n, const char** err) {
  VOXEL_REFUSE(n >= 0, "voxel_map_align: n must not be negative");
  VOXEL_REFUSE(n <= SVO_VOXEL_ALIGN_MAX_POINTS, "voxel_map_align: n beyond 2^20");
  return SVO_OK;
}

inline int voxel_align_points_check(const void* points, int n, const char** err) {  // n == 0: there is nothing to read
  if (n == 0) return SVO_OK;
  VOXEL_REFUSE(points, "voxel_map_align: null points");
  VOXEL_REFUSE(((uintptr_t)points & 3u) == 0, "voxel_map_align: points must be 4-byte aligned");
  return SVO_OK;
}

// The sums entries (the pose7 entry has checked n and refused its own null pose7 before).
inline int voxel_align_sums_check(const void* points, int n, const double* c2w12, const svo_voxel_align_params* p, const void* sums, const char** err) {
  if (const int rc = voxel_align_n_check(n, err)) return rc;
  VOXEL_REFUSE(c2w12, "voxel_map_align: null c2w12");
  if (const int rc = voxel_align_params_check(p, err)) return rc;
  VOXEL_REFUSE(sums, "voxel_map_align: null sums");
  VOXEL_REFUSE(((uintptr_t)sums & 7u) == 0, "voxel_map_align: sums must be 8-byte aligned");
  return voxel_align_points_check(points, n, err);
}

// The loop's entry (its sums are the library's own).
inline int voxel_align_loop_check(const void* points, int n, const double* pose7_in, const svo_voxel_align_params* p, const double* pose7_out,
                                  const svo_voxel_align_result* result, const char** err) {
  if (const int rc = voxel_align_n_check(n, err)) return rc;
  VOXEL_REFUSE(pose7_in, "voxel_map_align: null pose7_in");
  VOXEL_REFUSE(pose7_out, "voxel_map_align: null pose7_out");
  VOXEL_REFUSE(result, "voxel_map_align: null result");
  if (const int rc = voxel_align_params_check(p, err)) return rc;
  return voxel_align_points_check(points, n, err);
}

inline int voxel_align_default_params(float voxel_size, svo_voxel_align_params* p) {
  if (!p || !(voxel_size > 0.0f && voxel_size <= FLT_MAX)) return SVO_ERR_INVALID;
  const float twice = 2.0f * voxel_size;
  p->min_count = 1; p->reach = 1;
  p->max_dist = twice < VOXEL_ALIGN_MAX_DIST ? twice : VOXEL_ALIGN_MAX_DIST;
  p->max_iters = 10; p->min_matches = 64;
  p->eps_t = voxel_size / 100.0f; p->eps_r = 1e-5f;
  return SVO_OK;
}

// ----------------------------------------------------------------------------- pose7 <-> the camera->world (u, T)   (steps a, b, g)
inline void voxel_align_from_pose7(const double* pose7, double* u, double* T) {
  const double qw = pose7[0], qx = pose7[1], qy = pose7[2], qz = pose7[3];
  const double s = sqrt(qw * qw + qx * qx + qy * qy + qz * qz);
  u[0] = qw / s; u[1] = -qx / s; u[2] = -qy / s; u[3] = -qz / s;
  double R[9];
  voxel_quat_to_R(u, R);
  const double* t = pose7 + 4;
  for (int r = 0; r < 3; ++r) T[r] = -(R[3 * r] * t[0] + R[3 * r + 1] * t[1] + R[3 * r + 2] * t[2]);
}

inline void voxel_align_matrix(const double* u, const double* T, double* R, double* m12) {  // R: the 9 doubles the update needs
  voxel_quat_to_R(u, R);
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) m12[4 * r + c] = R[3 * r + c];
    m12[4 * r + 3] = T[r];
  }
}

inline void voxel_align_to_pose7(const double* u, const double* T, double* pose7) {
  double R[9];
  voxel_quat_to_R(u, R);
  pose7[0] = u[0]; pose7[1] = -u[1]; pose7[2] = -u[2]; pose7[3] = -u[3];
  for (int r = 0; r < 3; ++r) pose7[4 + r] = -(R[r] * T[0] + R[3 + r] * T[1] + R[6 + r] * T[2]);
}

// ----------------------------------------------------------------------------- H and g from the words   (step c)
inline void voxel_align_normal(const int64_t* w, double H[6][6], double g[6]) {
  const double N = (double)w[0];
  double A[3], B[6];  // B: 00 01 02 11 12 22
  for (int i = 0; i < 3; ++i) A[i] = (double)w[1 + i] / VOXEL_ALIGN_S16;
  for (int i = 0; i < 6; ++i) B[i] = (double)w[4 + i] / VOXEL_ALIGN_S16;
  for (int i = 0; i < 6; ++i) {
    for (int j = 0; j < 6; ++j) H[i][j] = 0.0;
    g[i] = (double)w[10 + i] / VOXEL_ALIGN_S28;
  }
  H[0][0] = N; H[1][1] = N; H[2][2] = N;
  H[0][4] = A[2]; H[0][5] = -A[1]; H[1][3] = -A[2]; H[1][5] = A[0]; H[2][3] = A[1]; H[2][4] = -A[0];
  H[3][3] = B[3] + B[5]; H[4][4] = B[0] + B[5]; H[5][5] = B[0] + B[3];
  H[3][4] = -B[1]; H[3][5] = -B[2]; H[4][5] = -B[4];
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < i; ++j) H[i][j] = H[j][i];
}

// H xi = -g by the unpivoted Cholesky factorisation of step d.  false: a pivot failed d > 0 && d <= DBL_MAX (xi is not written).
inline bool voxel_align_solve(const double H[6][6], const double g[6], double xi[6]) {
  double L[6][6], y[6], x[6];
  for (int j = 0; j < 6; ++j) {
    double d = H[j][j];
    for (int k = 0; k < j; ++k) d = d - L[j][k] * L[j][k];
    if (!(d > 0.0 && d <= DBL_MAX)) return false;
    L[j][j] = sqrt(d);
    for (int i = j + 1; i < 6; ++i) {
      double s = H[i][j];
      for (int k = 0; k < j; ++k) s = s - L[i][k] * L[j][k];
      L[i][j] = s / L[j][j];
    }
  }
  for (int i = 0; i < 6; ++i) {
    double s = -g[i];
    for (int k = 0; k < i; ++k) s = s - L[i][k] * y[k];
    y[i] = s / L[i][i];
  }
  for (int i = 5; i >= 0; --i) {
    double s = y[i];
    for (int k = i + 1; k < 6; ++k) s = s - L[k][i] * x[k];
    x[i] = s / L[i][i];
  }
  for (int i = 0; i < 6; ++i) xi[i] = x[i];
  return true;
}

// Step e: R is the matrix the sums were taken under.
inline void voxel_align_update(double* u, double* T, const double* R, const double* xi) {
  const double* v = xi;
  for (int r = 0; r < 3; ++r) T[r] = T[r] + (R[3 * r] * v[0] + R[3 * r + 1] * v[1] + R[3 * r + 2] * v[2]);
  const double b0 = xi[3] / 2.0, b1 = xi[4] / 2.0, b2 = xi[5] / 2.0;
  const double w = u[0] - u[1] * b0 - u[2] * b1 - u[3] * b2;
  const double x = u[1] + u[0] * b0 + u[2] * b2 - u[3] * b1;
  const double y = u[2] + u[0] * b1 - u[1] * b2 + u[3] * b0;
  const double z = u[3] + u[0] * b2 + u[1] * b1 - u[2] * b0;
  const double s = sqrt(w * w + x * x + y * y + z * z);
  const double a[4] = {w / s, x / s, y / s, z / s};
  // one first-order correction of the norm: the division alone leaves | |u| - 1 | at up to 1.5 ulp
  const double h = (1.0 - (a[0] * a[0] + a[1] * a[1] + a[2] * a[2] + a[3] * a[3])) / 2.0;
  for (int i = 0; i < 4; ++i) u[i] = a[i] + a[i] * h;
}

inline bool voxel_align_converged(const double* xi, const svo_voxel_align_params* p) {  // step f
  const double et = (double)p->eps_t * (double)p->eps_t, er = (double)p->eps_r * (double)p->eps_r;
  return xi[0] * xi[0] + xi[1] * xi[1] + xi[2] * xi[2] < et && xi[3] * xi[3] + xi[4] * xi[4] + xi[5] * xi[5] < er;
}

// The loop.  sums_at(m12, words) fills the 32 words of one matrix and returns SVO_OK, or an error code that ends the loop and is
// returned (pose7_out and result are then not written).  The arguments have passed voxel_align_loop_check.
template <typename SumsAt>
inline int voxel_align_loop(const double* pose7_in, const svo_voxel_align_params* p, SumsAt sums_at, double* pose7_out, svo_voxel_align_result* result) {
  double u[4], T[3], R[9], m12[12];
  voxel_align_from_pose7(pose7_in, u, T);
  svo_voxel_align_result res;
  memset(&res, 0, sizeof(res));
  res.status = SVO_VOXEL_ALIGN_MAX_ITERS;
  int steps = 0;
  for (int it = 0; it < p->max_iters; ++it) {
    int64_t w[VOXEL_ALIGN_WORDS];
    voxel_align_matrix(u, T, R, m12);
    if (const int rc = sums_at(m12, w)) return rc;
    res.iterations = it + 1;
    res.last_matched = w[VOXEL_ALIGN_COUNTS]; res.last_cost = w[16];
    if (it == 0) { res.first_matched = res.last_matched; res.first_cost = res.last_cost; }
    if (w[VOXEL_ALIGN_COUNTS] < (int64_t)p->min_matches) { res.status = SVO_VOXEL_ALIGN_TOO_FEW; break; }
    double H[6][6], g[6], xi[6];
    voxel_align_normal(w, H, g);
    if (!voxel_align_solve(H, g, xi)) { res.status = SVO_VOXEL_ALIGN_DEGENERATE; break; }
    voxel_align_update(u, T, R, xi);
    ++steps;
    for (int i = 0; i < 6; ++i) res.xi[i] = xi[i];
    if (voxel_align_converged(xi, p)) { res.status = SVO_VOXEL_ALIGN_CONVERGED; break; }
  }
  double out[7];
  if (steps) voxel_align_to_pose7(u, T, out);
  else memcpy(out, pose7_in, sizeof(out));
  memcpy(pose7_out, out, sizeof(out));
  *result = res;
  return SVO_OK;
}

inline size_t voxel_align_groups(int n) { return voxel_record_groups(n); }  // one record per thread

#endif  // SVO_VOXEL_ALIGN_H_
