// The voxel map normals' logic that needs no GPU (include/svo.h, "Voxel map normals"): the argument checks with their
// message texts and their order, the defaults, the side array's size, and - as __host__ __device__ inline code, so that the kernel
// of csrc/voxel_normals.hip and a CPU program run the same text - the integer moments of a neighbourhood, the fixed-sweep Jacobi,
// the validity tests and the output record.  A refusal is SVO_ERR_INVALID with *err set to the message.
// tests/sanitize/voxel_normals_args_test.cpp walks all of it on a CPU.
#ifndef SVO_VOXEL_NORMALS_H_
#define SVO_VOXEL_NORMALS_H_
#include <float.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "voxel_args.h"

constexpr size_t VOXEL_NORMAL_BYTES = 16;
constexpr int VOXEL_NORMALS_COUNTS = SVO_VOXEL_NORMALS_COUNTS;
constexpr int VOXEL_NORMALS_RUN = 16;    // slots per thread of the normals launch: a workgroup owns VOXEL_THREADS * 16 contiguous slots
constexpr int VOXEL_NORMALS_SWEEPS = 4;  // rule 4
enum { VOXEL_NORMAL_VALID = 0, VOXEL_NORMAL_FEW = 1, VOXEL_NORMAL_COLLINEAR = 2, VOXEL_NORMAL_CURVED = 3 };  // counts word 1 + verdict

// ----------------------------------------------------------------------------- the checks, in the contract's order
inline int voxel_normals_params_check(const svo_voxel_normals_params* p, const char** err) {
  VOXEL_REFUSE(p, "voxel_map_normals: null params");
  VOXEL_REFUSE(p->min_count >= 1, "voxel_map_normals: min_count must be at least 1");
  VOXEL_REFUSE(p->min_neighbours >= 3 && p->min_neighbours <= 27, "voxel_map_normals: min_neighbours outside 3..27");
  VOXEL_REFUSE(p->max_curvature > 0.0f && p->max_curvature <= 1.0f, "voxel_map_normals: max_curvature must be finite and in (0, 1]");  // a NaN fails the first test
  return SVO_OK;
}

// device: the _dev entry's pointers, whose alignment the kernel relies on; the synchronous entry copies into host pointers of any alignment.
inline int voxel_normals_check(const svo_voxel_normals_params* p, const void* normals, const void* counts, bool device, const char** err) {
  if (const int rc = voxel_normals_params_check(p, err)) return rc;
  VOXEL_REFUSE(normals, "voxel_map_normals: null normals");
  if (!device) return SVO_OK;
  VOXEL_REFUSE(((uintptr_t)normals & 15u) == 0, "voxel_map_normals: normals must be 16-byte aligned");
  VOXEL_REFUSE(((uintptr_t)counts & 7u) == 0, "voxel_map_normals: counts must be 8-byte aligned");
  return SVO_OK;
}

inline int voxel_normals_default_params(svo_voxel_normals_params* p) {
  if (!p) return SVO_ERR_INVALID;
  p->min_count = 1; p->min_neighbours = 5; p->max_curvature = 1.0f;
  return SVO_OK;
}

inline int voxel_normals_bytes(const svo_voxel_map_params* p, size_t* bytes) {
  if (!bytes) return SVO_ERR_INVALID;
  *bytes = 0;
  const char* err = nullptr;
  if (voxel_params_check(p, &err)) return SVO_ERR_INVALID;
  *bytes = VOXEL_NORMAL_BYTES << p->capacity_log2;
  return SVO_OK;
}

inline size_t voxel_normals_groups(size_t cap) { return voxel_div_up(cap, (size_t)VOXEL_THREADS * VOXEL_NORMALS_RUN); }

// ----------------------------------------------------------------------------- rule 3: the integer moments
struct VoxelMoments {
  long long n, s1[3], s2[6];  // s2: 00 01 02 11 12 22
};

VOXEL_HD inline void voxel_moments_clear(VoxelMoments& m) {
  m.n = 0;
  for (int i = 0; i < 3; ++i) m.s1[i] = 0;
  for (int i = 0; i < 6; ++i) m.s2[i] = 0;
}

// One participant: its offset (each of -1, 0, 1), its count (>= 1) and its three coordinate sums (each < 2^40).
VOXEL_HD inline void voxel_moments_add(VoxelMoments& m, int oi, int oj, int ol, unsigned count, unsigned long long sx, unsigned long long sy,
                                       unsigned long long sz) {
  const long long g0 = (long long)oi * 65536 + (long long)voxel_div40(sx, count);
  const long long g1 = (long long)oj * 65536 + (long long)voxel_div40(sy, count);
  const long long g2 = (long long)ol * 65536 + (long long)voxel_div40(sz, count);
  m.n += 1;
  m.s1[0] += g0; m.s1[1] += g1; m.s1[2] += g2;
  m.s2[0] += g0 * g0; m.s2[1] += g0 * g1; m.s2[2] += g0 * g2;
  m.s2[3] += g1 * g1; m.s2[4] += g1 * g2; m.s2[5] += g2 * g2;
}

// C_rs = N * S2_rs - S1_r * S1_s, as 00 01 02 11 12 22.
VOXEL_HD inline void voxel_moments_cov(const VoxelMoments& m, long long C[6]) {
  C[0] = m.n * m.s2[0] - m.s1[0] * m.s1[0]; C[1] = m.n * m.s2[1] - m.s1[0] * m.s1[1]; C[2] = m.n * m.s2[2] - m.s1[0] * m.s1[2];
  C[3] = m.n * m.s2[3] - m.s1[1] * m.s1[1]; C[4] = m.n * m.s2[4] - m.s1[1] * m.s1[2]; C[5] = m.n * m.s2[5] - m.s1[2] * m.s1[2];
}

// ----------------------------------------------------------------------------- rule 4: one Jacobi rotation, written without an index computed at run time
// app, aqq, apq: the pair's entries; arp, arq: the third index's; vNp, vNq: columns p and q of V.
#define VOXEL_JACOBI_PAIR(app, aqq, apq, arp, arq, v0p, v0q, v1p, v1q, v2p, v2q)      \
  do {                                                                                \
    if ((apq) != 0.0) {                                                               \
      const double th = ((aqq) - (app)) / (2.0 * (apq));                              \
      const double t = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));   \
      const double c = 1.0 / sqrt(t * t + 1.0);                                       \
      const double s = t * c;                                                         \
      const double x = t * (apq);                                                     \
      (app) = (app) - x; (aqq) = (aqq) + x; (apq) = 0.0;                              \
      double y = (arp), z = (arq);                                                    \
      (arp) = c * y - s * z; (arq) = s * y + c * z;                                   \
      y = (v0p); z = (v0q); (v0p) = c * y - s * z; (v0q) = s * y + c * z;             \
      y = (v1p); z = (v1q); (v1p) = c * y - s * z; (v1q) = s * y + c * z;             \
      y = (v2p); z = (v2q); (v2p) = c * y - s * z; (v2q) = s * y + c * z;             \
    }                                                                                 \
  } while (0)

// The eigenvalues (lambda) and eigenvectors (the columns of V, row-major V[3k + col]) of the symmetric matrix C (00 01 02 11 12 22).
VOXEL_HD inline void voxel_jacobi(const long long C[6], double lambda[3], double V[9]) {
  double a00 = (double)C[0], a01 = (double)C[1], a02 = (double)C[2], a11 = (double)C[3], a12 = (double)C[4], a22 = (double)C[5];
  double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
  for (int sweep = 0; sweep < VOXEL_NORMALS_SWEEPS; ++sweep) {
    VOXEL_JACOBI_PAIR(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);  // (0, 1), r = 2
    VOXEL_JACOBI_PAIR(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);  // (0, 2), r = 1
    VOXEL_JACOBI_PAIR(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);  // (1, 2), r = 0
  }
  lambda[0] = a00; lambda[1] = a11; lambda[2] = a22;
  V[0] = v00; V[1] = v01; V[2] = v02; V[3] = v10; V[4] = v11; V[5] = v12; V[6] = v20; V[7] = v21; V[8] = v22;
}

// ----------------------------------------------------------------------------- rules 5 and 6
VOXEL_HD inline void voxel_normal_none(svo_voxel_normal* out) { out->nx = 0.0f; out->ny = 0.0f; out->nz = 0.0f; out->curvature = -1.0f; }

// The record of a centre from its moments; returns the verdict (VOXEL_NORMAL_*).  p has passed voxel_normals_params_check.
VOXEL_HD inline int voxel_normal_finish(const VoxelMoments& m, int min_neighbours, float max_curvature, svo_voxel_normal* out) {
  voxel_normal_none(out);
  if (m.n < (long long)min_neighbours) return VOXEL_NORMAL_FEW;
  long long C[6];
  voxel_moments_cov(m, C);
  double l[3], V[9];
  voxel_jacobi(C, l, V);
  // lo: the lowest index with the smallest lambda; mid: of the other two the smaller (the lower index if equal)
  const int lo = l[1] < l[0] ? (l[2] < l[1] ? 2 : 1) : (l[2] < l[0] ? 2 : 0);
  const int o0 = lo == 0 ? 1 : 0, o1 = lo == 2 ? 1 : 2;
  const double l_lo = lo == 0 ? l[0] : (lo == 1 ? l[1] : l[2]);
  const double l_o0 = o0 == 0 ? l[0] : l[1], l_o1 = o1 == 1 ? l[1] : l[2];
  const double l_mid = l_o1 < l_o0 ? l_o1 : l_o0;
  const double tr = l[0] + l[1] + l[2];
  if (!(l_mid > 0.0)) return VOXEL_NORMAL_COLLINEAR;
  const double low = l_lo > 0.0 ? l_lo : 0.0;
  if (!(low <= (double)max_curvature * tr)) return VOXEL_NORMAL_CURVED;
  double n0 = lo == 0 ? V[0] : (lo == 1 ? V[1] : V[2]);
  double n1 = lo == 0 ? V[3] : (lo == 1 ? V[4] : V[5]);
  double n2 = lo == 0 ? V[6] : (lo == 1 ? V[7] : V[8]);
  const double f0 = fabs(n0), f1 = fabs(n1), f2 = fabs(n2);
  const double lead = f1 > f0 ? (f2 > f1 ? n2 : n1) : (f2 > f0 ? n2 : n0);  // the lowest index of the largest magnitude
  if (lead < 0.0) { n0 = -n0; n1 = -n1; n2 = -n2; }
  out->nx = (float)n0; out->ny = (float)n1; out->nz = (float)n2;
  out->curvature = (float)(low / tr);
  return VOXEL_NORMAL_VALID;
}

#endif  // SVO_VOXEL_NORMALS_H_
