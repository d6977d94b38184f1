// The voxel map locate's host logic that needs no GPU (include/svo.h, "Voxel map locate"): the argument checks with
// their message texts and their order, the defaults, the sizes, the candidates' quaternions and matrices, the volume's origin,
// the ranking, the selection and the whole loop over two functors (the scores of K matrices, and the refinement of one pose7).
// Only + - * / and sqrt on doubles in the written order, as host/voxel_align.h, whose steps a, g and R(u) it calls.
// A candidate's turn is a = (1, b e_axis) / |.| with b = j * turn_step / 2: its angle is 2 atan(b), NOT j * turn_step, so no
// trigonometric function is needed and a restatement in another language gives the same bits.
// A refusal is SVO_ERR_INVALID with *err set to the message; csrc/voxel_locate.hip stores it in the context, supplies the functors
// and keeps no second copy of anything here.  tests/sanitize/voxel_locate_args_test.cpp walks all of it on a CPU.
#ifndef SVO_VOXEL_LOCATE_H_
#define SVO_VOXEL_LOCATE_H_
#include "voxel_align.h"

constexpr int VOXEL_LOCATE_MAX_K = SVO_VOXEL_LOCATE_MAX_K, VOXEL_LOCATE_MAX_BOX = SVO_VOXEL_LOCATE_MAX_BOX;
constexpr int VOXEL_LOCATE_KEY_LO = -(1 << 20), VOXEL_LOCATE_KEY_HI = 1 << 20;  // the key range [LO, HI)
constexpr double VOXEL_LOCATE_LIMIT = 1048560.0;                               // rule 1: sixteen voxels inside the key range
constexpr int VOXEL_OCCUPANCY_THREADS = 1024;                                  // the occupancy walk's workgroup: fewer adds to its two counts
constexpr int VOXEL_LOCATE_CHUNK = 1024;                                       // records per workgroup of the score launch
constexpr int VOXEL_LOCATE_LAUNCH_K = 32;                                      // candidates per score launch: 32 * 96 bytes of arguments

// ----------------------------------------------------------------------------- the checks, in the contract's order
inline int voxel_occupancy_origin_check(const int* origin, const char** err) {
  VOXEL_REFUSE(origin, "voxel_map_occupancy: null origin");
  for (int r = 0; r < 3; ++r) VOXEL_REFUSE(origin[r] >= VOXEL_LOCATE_KEY_LO && origin[r] < VOXEL_LOCATE_KEY_HI, "voxel_map_occupancy: origin outside [-2^20, 2^20)");
  return SVO_OK;
}

inline int voxel_occupancy_dims_check(const int* dims, const char** err) {
  VOXEL_REFUSE(dims, "voxel_map_occupancy: null dims");
  for (int r = 0; r < 3; ++r) VOXEL_REFUSE(dims[r] >= 1 && dims[r] <= 2048, "voxel_map_occupancy: dims outside 1..2048");
  VOXEL_REFUSE((dims[0] & 63) == 0, "voxel_map_occupancy: dims[0] must be a multiple of 64");
  VOXEL_REFUSE((long long)dims[0] * dims[1] * dims[2] <= (1ll << 30), "voxel_map_occupancy: dims[0] * dims[1] * dims[2] beyond 2^30");
  return SVO_OK;
}

inline size_t voxel_occupancy_words(const int* dims) { return (size_t)dims[0] / 64 * (size_t)dims[1] * (size_t)dims[2]; }  // dims are checked

inline int voxel_occupancy_bytes(const int* dims, size_t* bytes) {
  if (!bytes) return SVO_ERR_INVALID;
  *bytes = 0;
  const char* err = nullptr;
  if (voxel_occupancy_dims_check(dims, &err)) return SVO_ERR_INVALID;
  *bytes = 8 * voxel_occupancy_words(dims);
  return SVO_OK;
}

inline int voxel_occupancy_bits_check(const void* bits, const char** err) {
  VOXEL_REFUSE(bits, "voxel_map_occupancy: null bits");
  VOXEL_REFUSE(((uintptr_t)bits & 7u) == 0, "voxel_map_occupancy: bits must be 8-byte aligned");
  return SVO_OK;
}

// device: the _dev entry's pointers, whose alignment the kernel relies on; the host form's counts may be null and of any alignment.
inline int voxel_occupancy_check(int min_count, const int* origin, const int* dims, const void* bits, const void* counts, bool device, const char** err) {
  VOXEL_REFUSE(min_count >= 1, "voxel_map_occupancy: min_count must be at least 1");
  if (const int rc = voxel_occupancy_origin_check(origin, err)) return rc;
  if (const int rc = voxel_occupancy_dims_check(dims, err)) return rc;
  if (!device) { VOXEL_REFUSE(bits, "voxel_map_occupancy: null bits"); return SVO_OK; }
  if (const int rc = voxel_occupancy_bits_check(bits, err)) return rc;
  VOXEL_REFUSE(counts, "voxel_map_occupancy: null counts");
  VOXEL_REFUSE(((uintptr_t)counts & 3u) == 0, "voxel_map_occupancy: counts must be 4-byte aligned");
  return SVO_OK;
}

inline int voxel_locate_box_check(const int* box, const char** err) {
  for (int r = 0; r < 3; ++r) VOXEL_REFUSE(box[r] >= 0 && box[r] <= VOXEL_LOCATE_MAX_BOX, "voxel_map_locate: box outside 0..16");
  return SVO_OK;
}

inline size_t voxel_locate_shifts(const int* box) { return (size_t)(2 * box[0] + 1) * (size_t)(2 * box[1] + 1) * (size_t)(2 * box[2] + 1); }

inline int voxel_locate_scores_check(const void* bits, const int* origin, const int* dims, const void* points, int n, const double* mats, int K,
                                     const int* box, const void* hits, const void* best, const char** err) {
  VOXEL_REFUSE(n >= 0, "voxel_map_locate: n must not be negative");
  VOXEL_REFUSE(n <= SVO_VOXEL_ALIGN_MAX_POINTS, "voxel_map_locate: n beyond 2^20");
  VOXEL_REFUSE(mats, "voxel_map_locate: null mats");
  VOXEL_REFUSE(K >= 1 && K <= VOXEL_LOCATE_MAX_K, "voxel_map_locate: K outside 1..63");
  VOXEL_REFUSE(box, "voxel_map_locate: null box");
  if (const int rc = voxel_locate_box_check(box, err)) return rc;
  if (const int rc = voxel_occupancy_origin_check(origin, err)) return rc;
  if (const int rc = voxel_occupancy_dims_check(dims, err)) return rc;
  if (const int rc = voxel_occupancy_bits_check(bits, err)) return rc;
  VOXEL_REFUSE(hits, "voxel_map_locate: null hits");
  VOXEL_REFUSE(((uintptr_t)hits & 3u) == 0, "voxel_map_locate: hits must be 4-byte aligned");
  VOXEL_REFUSE(best, "voxel_map_locate: null best");
  VOXEL_REFUSE(((uintptr_t)best & 7u) == 0, "voxel_map_locate: best must be 8-byte aligned");
  if (n == 0) return SVO_OK;
  VOXEL_REFUSE(points, "voxel_map_locate: null points");
  VOXEL_REFUSE(((uintptr_t)points & 3u) == 0, "voxel_map_locate: points must be 4-byte aligned");
  return SVO_OK;
}

inline int voxel_locate_params_check(const svo_voxel_locate_params* p, const char** err) {
  VOXEL_REFUSE(p, "voxel_map_locate: null params");
  VOXEL_REFUSE(p->min_count >= 1, "voxel_map_locate: min_count must be at least 1");
  VOXEL_REFUSE(p->up_axis >= 0 && p->up_axis <= 2, "voxel_map_locate: up_axis outside 0..2");
  VOXEL_REFUSE(p->n_turn >= 0 && p->n_turn <= 31, "voxel_map_locate: n_turn outside 0..31");
  VOXEL_REFUSE(p->turn_step > 0.0f && p->turn_step <= 0.25f, "voxel_map_locate: turn_step must be finite and in (0, 0.25]");  // a NaN fails the first test
  if (const int rc = voxel_locate_box_check(p->box, err)) return rc;
  if (const int rc = voxel_occupancy_dims_check(p->dims, err)) return rc;
  VOXEL_REFUSE(p->n_refine >= 1 && p->n_refine <= VOXEL_LOCATE_MAX_K, "voxel_map_locate: n_refine outside 1..63");
  VOXEL_REFUSE(p->min_hits >= 1, "voxel_map_locate: min_hits must be at least 1");
  return SVO_OK;
}

inline int voxel_locate_loop_check(const void* normals, const void* points, int n, const double* pose7_in, const svo_voxel_locate_params* p,
                                   const svo_voxel_align_params* ap, const void* workspace, const double* pose7_out,
                                   const svo_voxel_locate_result* result, const char** err) {
  VOXEL_REFUSE(n >= 0, "voxel_map_locate: n must not be negative");
  VOXEL_REFUSE(n <= SVO_VOXEL_ALIGN_MAX_POINTS, "voxel_map_locate: n beyond 2^20");
  VOXEL_REFUSE(pose7_in, "voxel_map_locate: null pose7_in");
  VOXEL_REFUSE(pose7_out, "voxel_map_locate: null pose7_out");
  VOXEL_REFUSE(result, "voxel_map_locate: null result");
  if (const int rc = voxel_locate_params_check(p, err)) return rc;
  if (const int rc = voxel_align_params_check(ap, err)) return rc;
  VOXEL_REFUSE(workspace, "voxel_map_locate: null workspace");
  VOXEL_REFUSE(((uintptr_t)workspace & 255u) == 0, "voxel_map_locate: workspace must be 256-byte aligned");
  VOXEL_REFUSE(((uintptr_t)normals & 15u) == 0, "voxel_map_locate: normals must be 16-byte aligned");
  if (n == 0) return SVO_OK;
  VOXEL_REFUSE(points, "voxel_map_locate: null points");
  VOXEL_REFUSE(((uintptr_t)points & 3u) == 0, "voxel_map_locate: points must be 4-byte aligned");
  return SVO_OK;
}

inline int voxel_locate_default_params(float voxel_size, svo_voxel_locate_params* p) {
  if (!p || !(voxel_size > 0.0f && voxel_size <= FLT_MAX)) return SVO_ERR_INVALID;
  p->min_count = 1; p->up_axis = 1; p->n_turn = 4; p->turn_step = 0.04f;
  p->box[0] = 8; p->box[1] = 4; p->box[2] = 8;
  p->dims[0] = 512; p->dims[1] = 128; p->dims[2] = 512;
  p->n_refine = 3; p->min_hits = 64;
  return SVO_OK;
}

// ----------------------------------------------------------------------------- the workspace: volume | counts | scores | bests
struct VoxelLocateLayout { size_t bits, counts, hits, best, total; };
inline size_t voxel_locate_round(size_t b) { return (b + 255) & ~(size_t)255; }

inline VoxelLocateLayout voxel_locate_layout(const svo_voxel_locate_params* p) {  // p has passed voxel_locate_params_check
  const size_t K = (size_t)(2 * p->n_turn + 1);
  VoxelLocateLayout l;
  l.bits = 0;
  l.counts = voxel_locate_round(8 * voxel_occupancy_words(p->dims));
  l.hits = l.counts + 256;
  l.best = l.hits + voxel_locate_round(4 * K * voxel_locate_shifts(p->box));
  l.total = l.best + voxel_locate_round(K * sizeof(svo_voxel_locate_best));
  return l;
}

inline int voxel_locate_workspace_bytes(const svo_voxel_locate_params* p, size_t* bytes) {
  if (!bytes) return SVO_ERR_INVALID;
  *bytes = 0;
  const char* err = nullptr;
  if (voxel_locate_params_check(p, &err)) return SVO_ERR_INVALID;
  *bytes = voxel_locate_layout(p).total;
  return SVO_OK;
}

// ----------------------------------------------------------------------------- step b: the candidates
inline void voxel_locate_turn(const double* u, int axis, double b, double* uk) {
  const double nrm = sqrt(1.0 + b * b);
  double a[4] = {1.0 / nrm, 0.0, 0.0, 0.0};
  a[1 + axis] = b / nrm;
  const double w = a[0] * u[0] - a[1] * u[1] - a[2] * u[2] - a[3] * u[3];
  const double x = a[0] * u[1] + a[1] * u[0] + a[2] * u[3] - a[3] * u[2];
  const double y = a[0] * u[2] - a[1] * u[3] + a[2] * u[0] + a[3] * u[1];
  const double z = a[0] * u[3] + a[1] * u[2] - a[2] * u[1] + a[3] * u[0];
  const double s = sqrt(w * w + x * x + y * y + z * z);
  const double c[4] = {w / s, x / s, y / s, z / s};
  const double h = (1.0 - (c[0] * c[0] + c[1] * c[1] + c[2] * c[2] + c[3] * c[3])) / 2.0;  // the align's first-order correction
  for (int i = 0; i < 4; ++i) uk[i] = c[i] + c[i] * h;
}

inline void voxel_locate_candidate(const double* u, const double* T, const svo_voxel_locate_params* p, int k, double* uk, double* m12) {
  const double b = ((double)(k - p->n_turn) * (double)p->turn_step) / 2.0;
  voxel_locate_turn(u, p->up_axis, b, uk);
  double R[9];
  voxel_align_matrix(uk, T, R, m12);
}

// ----------------------------------------------------------------------------- step c: the volume's origin
inline int voxel_locate_origin(const double* T, float voxel_size, const int* dims, int* origin, const char** err) {
  for (int r = 0; r < 3; ++r) {
    const double f = floor(T[r] / (double)voxel_size);
    VOXEL_REFUSE(f >= -2097152.0 && f <= 2097152.0, "voxel_map_locate: the prior's position is outside the key range");  // a NaN fails
    const int o = (int)f - dims[r] / 2;
    VOXEL_REFUSE(o >= VOXEL_LOCATE_KEY_LO && o + dims[r] <= VOXEL_LOCATE_KEY_HI, "voxel_map_locate: the volume around the prior leaves the key range");
    origin[r] = o;
  }
  return SVO_OK;
}

// ----------------------------------------------------------------------------- step e: the ranking
// order[0..return): the candidates with hits_max >= min_hits by descending hits_max, ties by ascending k.
inline int voxel_locate_rank(const svo_voxel_locate_best* best, int K, int min_hits, int* order) {
  int m = 0;
  for (int k = 0; k < K; ++k) {
    if (best[k].hits_max < (uint32_t)min_hits) continue;
    int at = m++;
    for (; at > 0 && best[order[at - 1]].hits_max < best[k].hits_max; --at) order[at] = order[at - 1];  // equal scores: the earlier k stays in front
    order[at] = k;
  }
  return m;
}

// Step g's order: is refinement a (of a later rank) better than the best so far, b?
inline bool voxel_locate_better(const svo_voxel_align_result& a, const svo_voxel_align_result& b) {
  return a.last_matched > b.last_matched || (a.last_matched == b.last_matched && a.last_cost < b.last_cost);
}

inline bool voxel_locate_eligible(const svo_voxel_align_result& a) { return a.status == SVO_VOXEL_ALIGN_CONVERGED || a.status == SVO_VOXEL_ALIGN_MAX_ITERS; }

// The loop.  scores_at(mats, K, origin, best) fills the K bests of the K matrices (steps c's volume and d) and refine(pose7, out, res)
// runs one align; both return SVO_OK or an error code that ends the loop and is returned (pose7_out and result are then not
// written).  The arguments have passed voxel_locate_loop_check.
template <typename ScoresAt, typename Refine>
inline int voxel_locate_loop(const double* pose7_in, const svo_voxel_locate_params* p, float voxel_size, ScoresAt scores_at, Refine refine, double* pose7_out,
                             svo_voxel_locate_result* result, const char** err) {
  double u[4], T[3];
  voxel_align_from_pose7(pose7_in, u, T);
  const int K = 2 * p->n_turn + 1;
  double uk[VOXEL_LOCATE_MAX_K][4], mats[VOXEL_LOCATE_MAX_K * 12];
  for (int k = 0; k < K; ++k) voxel_locate_candidate(u, T, p, k, uk[k], mats + 12 * k);
  int origin[3];
  if (const int rc = voxel_locate_origin(T, voxel_size, p->dims, origin, err)) return rc;
  svo_voxel_locate_best best[VOXEL_LOCATE_MAX_K];
  if (const int rc = scores_at(mats, K, origin, best)) return rc;
  int order[VOXEL_LOCATE_MAX_K];
  const int m = voxel_locate_rank(best, K, p->min_hits, order);
  svo_voxel_locate_result res;
  memset(&res, 0, sizeof(res));
  double out[7];
  if (m == 0) {
    res.status = SVO_VOXEL_LOCATE_NO_CANDIDATE; res.k = -1; res.rank = -1;
    memcpy(out, pose7_in, sizeof(out));
    memcpy(res.coarse_pose7, pose7_in, sizeof(out));
  } else {
    const int tries = m < p->n_refine ? m : p->n_refine;
    int chosen = -1;
    double coarse0[7];
    svo_voxel_align_result first;
    for (int i = 0; i < tries; ++i) {
      const svo_voxel_locate_best& b = best[order[i]];
      const int s[3] = {b.s0, b.s1, b.s2};
      double Tk[3], coarse[7], fine[7];
      for (int r = 0; r < 3; ++r) Tk[r] = T[r] + (double)s[r] * (double)voxel_size;
      voxel_align_to_pose7(uk[order[i]], Tk, coarse);
      svo_voxel_align_result ar;
      if (const int rc = refine(coarse, fine, &ar)) return rc;
      if (i == 0) { memcpy(coarse0, coarse, sizeof(coarse)); first = ar; }
      if (voxel_locate_eligible(ar) && (chosen < 0 || voxel_locate_better(ar, res.align))) {
        chosen = i;
        res.align = ar;
        memcpy(res.coarse_pose7, coarse, sizeof(coarse));
        memcpy(out, fine, sizeof(fine));
      }
    }
    res.n_refined = tries;
    if (chosen < 0) {
      res.status = SVO_VOXEL_LOCATE_UNREFINED;
      chosen = 0;
      res.align = first;
      memcpy(res.coarse_pose7, coarse0, sizeof(coarse0));
      memcpy(out, coarse0, sizeof(coarse0));
    } else {
      res.status = SVO_VOXEL_LOCATE_FOUND;
    }
    const svo_voxel_locate_best& b = best[order[chosen]];
    res.k = order[chosen]; res.rank = chosen; res.hits = b.hits_max;
    res.shift[0] = b.s0; res.shift[1] = b.s1; res.shift[2] = b.s2;
  }
  memcpy(pose7_out, out, sizeof(out));
  *result = res;
  return SVO_OK;
}

// ----------------------------------------------------------------------------- launch geometry
inline size_t voxel_occupancy_groups(size_t cap) { return voxel_div_up(cap, VOXEL_OCCUPANCY_THREADS); }  // one slot per thread
inline size_t voxel_locate_chunks(int n) { return voxel_div_up((size_t)n, VOXEL_LOCATE_CHUNK); }

#endif  // SVO_VOXEL_LOCATE_H_
