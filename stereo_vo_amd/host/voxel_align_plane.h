// The plane form of the voxel map align (include/svo.h, "Voxel map align, plane form"), the part that needs no GPU: the
// argument checks (the align's, with the normals' two directly after the null map), a match's 28 quantised terms as __host__
// __device__ inline code (the kernel of csrc/voxel_align_plane.hip and a CPU program run the same text), the assembly of H and g
// from the 40 words, and the loop.  Steps a, b, d, e, f and g of the loop are host/voxel_align.h's functions, called here.
// tests/sanitize/voxel_normals_args_test.cpp walks all of it on a CPU.
#ifndef SVO_VOXEL_ALIGN_PLANE_H_
#define SVO_VOXEL_ALIGN_PLANE_H_
#include "voxel_align.h"

#if defined(__HIPCC__)
#define VOXEL_UNROLL _Pragma("unroll")  // the kernel indexes no array at run time; a host compiler needs no hint
#else
#define VOXEL_UNROLL
#endif

constexpr int VOXEL_ALIGN_PLANE_WORDS = SVO_VOXEL_ALIGN_PLANE_WORDS;
constexpr int VOXEL_ALIGN_PLANE_TERMS = 28;   // words 1..28
constexpr int VOXEL_ALIGN_PLANE_COST = 28;    // the word of r * r
constexpr int VOXEL_ALIGN_PLANE_COUNTS = 29;  // words 29..33: n_matched, n_rejected, n_unmatched, n_far, n_no_normal
constexpr double VOXEL_ALIGN_S20 = 1048576.0, VOXEL_ALIGN_S30 = 1073741824.0, VOXEL_ALIGN_S36 = 68719476736.0, VOXEL_ALIGN_S40 = 1099511627776.0;

// ----------------------------------------------------------------------------- the checks, in the contract's order
inline int voxel_align_plane_normals_check(const void* normals, const char** err) {
  VOXEL_REFUSE(normals, "voxel_map_align_plane: null normals");
  VOXEL_REFUSE(((uintptr_t)normals & 15u) == 0, "voxel_map_align_plane: normals must be 16-byte aligned");
  return SVO_OK;
}

inline int voxel_align_plane_sums_check(const void* normals, const void* points, int n, const double* c2w12, const svo_voxel_align_params* p,
                                        const void* sums, const char** err) {
  if (const int rc = voxel_align_plane_normals_check(normals, err)) return rc;
  return voxel_align_sums_check(points, n, c2w12, p, sums, err);
}

inline int voxel_align_plane_loop_check(const void* normals, const void* points, int n, const double* pose7_in, const svo_voxel_align_params* p,
                                        const double* pose7_out, const svo_voxel_align_result* result, const char** err) {
  if (const int rc = voxel_align_plane_normals_check(normals, err)) return rc;
  return voxel_align_loop_check(points, n, pose7_in, p, pose7_out, result, err);
}

// ----------------------------------------------------------------------------- rule 4': the word and the scale of j_i * j_k, i <= k
VOXEL_HD constexpr int voxel_align_plane_word(int i, int k) { return 1 + 6 * i - i * (i - 1) / 2 + (k - i); }
VOXEL_HD constexpr double voxel_align_plane_scale(int i, int k) { return k < 3 ? VOXEL_ALIGN_S40 : (i < 3 ? VOXEL_ALIGN_S30 : VOXEL_ALIGN_S20); }

// The terms of one contributing match: v[t] is word 1 + t.  nn: the normal, e: the world-frame residual, m: the 12 doubles of the
// matrix, P: the record.
VOXEL_HD inline void voxel_align_plane_terms(const double nn[3], const double e[3], const double* m, const double P[3], long long v[VOXEL_ALIGN_PLANE_TERMS]) {
  const double r = nn[0] * e[0] + nn[1] * e[1] + nn[2] * e[2];
  double j[6];
VOXEL_UNROLL
  for (int c = 0; c < 3; ++c) j[c] = m[c] * nn[0] + m[4 + c] * nn[1] + m[8 + c] * nn[2];
  j[3] = P[1] * j[2] - P[2] * j[1];
  j[4] = P[2] * j[0] - P[0] * j[2];
  j[5] = P[0] * j[1] - P[1] * j[0];
VOXEL_UNROLL
  for (int i = 0; i < 6; ++i) {
VOXEL_UNROLL
    for (int k = i; k < 6; ++k) v[voxel_align_plane_word(i, k) - 1] = voxel_align_q(j[i] * j[k], voxel_align_plane_scale(i, k));
  }
VOXEL_UNROLL
  for (int i = 0; i < 3; ++i) {
    v[21 + i] = voxel_align_q(j[i] * r, VOXEL_ALIGN_S36);
    v[24 + i] = voxel_align_q(j[3 + i] * r, VOXEL_ALIGN_S28);
  }
  v[27] = voxel_align_q(r * r, VOXEL_ALIGN_S28);
}

// ----------------------------------------------------------------------------- step c': H and g from the words
inline void voxel_align_plane_normal(const int64_t* w, double H[6][6], double g[6]) {
  for (int i = 0; i < 6; ++i)
    for (int k = i; k < 6; ++k) H[i][k] = H[k][i] = (double)w[voxel_align_plane_word(i, k)] / voxel_align_plane_scale(i, k);
  for (int i = 0; i < 3; ++i) {
    g[i] = (double)w[22 + i] / VOXEL_ALIGN_S36;
    g[3 + i] = (double)w[25 + i] / VOXEL_ALIGN_S28;
  }
}

// The loop.  sums_at(m12, words) fills the 40 words of one matrix and returns SVO_OK, or an error code that ends the loop and is
// returned (pose7_out and result are then not written).  The arguments have passed voxel_align_plane_loop_check.
template <typename SumsAt>
inline int voxel_align_plane_loop(const double* pose7_in, const svo_voxel_align_params* p, SumsAt sums_at, double* pose7_out,
                                  svo_voxel_align_result* result) {
  double u[4], T[3], R[9], m12[12];
  voxel_align_from_pose7(pose7_in, u, T);
  svo_voxel_align_result res;
  memset(&res, 0, sizeof(res));
  res.status = SVO_VOXEL_ALIGN_MAX_ITERS;
  int steps = 0;
  for (int it = 0; it < p->max_iters; ++it) {
    int64_t w[VOXEL_ALIGN_PLANE_WORDS];
    voxel_align_matrix(u, T, R, m12);
    if (const int rc = sums_at(m12, w)) return rc;
    res.iterations = it + 1;
    res.last_matched = w[VOXEL_ALIGN_PLANE_COUNTS]; res.last_cost = w[VOXEL_ALIGN_PLANE_COST];
    if (it == 0) { res.first_matched = res.last_matched; res.first_cost = res.last_cost; }
    if (w[VOXEL_ALIGN_PLANE_COUNTS] < (int64_t)p->min_matches) { res.status = SVO_VOXEL_ALIGN_TOO_FEW; break; }
    double H[6][6], g[6], xi[6];
    voxel_align_plane_normal(w, H, g);
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

#endif  // SVO_VOXEL_ALIGN_PLANE_H_
