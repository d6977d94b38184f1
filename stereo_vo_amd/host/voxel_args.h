// The voxel map's host logic that needs no GPU (include/svo.h, "voxel map"): the parameter test and the table's
// size, pose7 -> the two 3 x 4 matrices, the argument checks of the cloud, carve, render and grid entries, the copy's box -> key
// range, the grid's conversions, cell rule and exact division, and the launch geometry.  A refusal is SVO_ERR_INVALID with *err set
// to the message; csrc/voxel.hip stores it in the context and keeps no second copy of anything here.
// tests/sanitize/voxel_args_test.cpp and voxel_grid_args_test.cpp walk every refusal at its boundary on a CPU.
#ifndef SVO_VOXEL_ARGS_H_
#define SVO_VOXEL_ARGS_H_
#include <float.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "svo.h"

#define VOXEL_REFUSE(cond, msg) do { if (!(cond)) { *err = (msg); return SVO_ERR_INVALID; } } while (0)

constexpr size_t VOXEL_SLOT_BYTES = 40;  // key, count | intensity sum, three coordinate sums
constexpr int VOXEL_THREADS = 256;       // every voxel kernel's workgroup
constexpr int VOXEL_WALK_ITEMS = 8;      // slots per thread of a launch that walks the table
constexpr int VOXEL_RESOLVE_PIXELS = 4;  // pixels per thread of the render's resolve

// ----------------------------------------------------------------------------- the map's parameters
inline int voxel_params_check(const svo_voxel_map_params* p, const char** err) {
  VOXEL_REFUSE(p, "voxel_map_create: null params");
  VOXEL_REFUSE(p->voxel_size > 0.0f && p->voxel_size <= FLT_MAX, "voxel_map_create: voxel_size must be finite and > 0");  // a NaN fails the first test
  VOXEL_REFUSE(p->capacity_log2 >= 8 && p->capacity_log2 <= 28, "voxel_map_create: capacity_log2 outside 8..28");
  return SVO_OK;
}

inline int voxel_table_bytes(const svo_voxel_map_params* p, size_t* bytes) {
  if (!bytes) return SVO_ERR_INVALID;
  *bytes = 0;
  const char* err = nullptr;
  if (voxel_params_check(p, &err)) return SVO_ERR_INVALID;
  *bytes = VOXEL_SLOT_BYTES << p->capacity_log2;
  return SVO_OK;
}

// ----------------------------------------------------------------------------- pose7 = [qw qx qy qz tx ty tz], X_cam = R(q) X_world + t
inline void voxel_quat_to_R(const double* q, double* R) {  // s = 2 / |q|^2: q need not be a unit quaternion
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  const double s = 2.0 / (w * w + x * x + y * y + z * z);
  R[0] = 1.0 - s * (y * y + z * z); R[1] = s * (x * y - w * z); R[2] = s * (x * z + w * y);
  R[3] = s * (x * y + w * z); R[4] = 1.0 - s * (x * x + z * z); R[5] = s * (y * z - w * x);
  R[6] = s * (x * z - w * y); R[7] = s * (y * z + w * x); R[8] = 1.0 - s * (x * x + y * y);
}

inline void voxel_pose7_to_cam_to_world(const double* pose7, double* m12) {  // [R^T | -R^T t]
  double R[9];
  voxel_quat_to_R(pose7, R);
  const double* t = pose7 + 4;
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) m12[4 * r + c] = R[3 * c + r];
    m12[4 * r + 3] = -(R[r] * t[0] + R[3 + r] * t[1] + R[6 + r] * t[2]);
  }
}

inline void voxel_pose7_to_world_to_cam(const double* pose7, double* m12) {  // [R | t]
  double R[9];
  voxel_quat_to_R(pose7, R);
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) m12[4 * r + c] = R[3 * r + c];
    m12[4 * r + 3] = pose7[4 + r];
  }
}

// ----------------------------------------------------------------------------- the entries that take a cloud (insert, removal, move)
struct VoxelCloudTexts { const char *negative_n, *null_matrix, *null_points, *points_alignment, *counts_alignment; };
#define VOXEL_CLOUD_TEXTS(what, matrix) \
  {what ": n must not be negative", what ": null " matrix, what ": null points", what ": points must be 4-byte aligned", what ": counts must be 8-byte aligned"}
constexpr VoxelCloudTexts VOXEL_INSERT_TEXTS = VOXEL_CLOUD_TEXTS("voxel_map_insert", "m12");
constexpr VoxelCloudTexts VOXEL_REMOVE_TEXTS = VOXEL_CLOUD_TEXTS("voxel_map_remove", "m12");
constexpr VoxelCloudTexts VOXEL_MOVE_TEXTS = VOXEL_CLOUD_TEXTS("voxel_map_move", "from_m12");

// n == 0 is accepted with null points: there is nothing to read.
inline int voxel_cloud_check(const void* points, int n, const double* m12, const VoxelCloudTexts& t, const char** err) {
  VOXEL_REFUSE(n >= 0, t.negative_n);
  VOXEL_REFUSE(m12, t.null_matrix);
  if (n == 0) return SVO_OK;
  VOXEL_REFUSE(points, t.null_points);
  VOXEL_REFUSE(((uintptr_t)points & 3u) == 0, t.points_alignment);
  return SVO_OK;
}

inline int voxel_counts_check(const void* counts, const VoxelCloudTexts& t, const char** err) {  // null: no counts wanted
  VOXEL_REFUSE(((uintptr_t)counts & 7u) == 0, t.counts_alignment);
  return SVO_OK;
}

// ----------------------------------------------------------------------------- carve and render (max_width, max_height: the context's limits)
inline int voxel_carve_check(const void* disp16, int width, int height, const svo_camera_info* cam, const double* w2c12,
                             const svo_voxel_carve_params* prm, int max_width, int max_height, const char** err) {
  VOXEL_REFUSE(disp16, "voxel_map_carve: null disp16");
  VOXEL_REFUSE(cam, "voxel_map_carve: null cam");
  VOXEL_REFUSE(w2c12, "voxel_map_carve: null w2c12");
  VOXEL_REFUSE(prm, "voxel_map_carve: null params");
  VOXEL_REFUSE(prm->radius >= 0 && prm->radius <= 3, "voxel_map_carve: radius outside 0..3");
  VOXEL_REFUSE(prm->margin16 >= 0 && prm->margin16 <= 32767, "voxel_map_carve: margin16 outside 0..32767");
  VOXEL_REFUSE(prm->keep_count >= 0, "voxel_map_carve: keep_count must not be negative");
  VOXEL_REFUSE(width >= 2 * prm->radius + 1 && width <= max_width, "voxel_map_carve: width below 2 radius + 1 or beyond the context's limit");
  VOXEL_REFUSE(height >= 2 * prm->radius + 1 && height <= max_height, "voxel_map_carve: height below 2 radius + 1 or beyond the context's limit");
  VOXEL_REFUSE(cam->focal != 0.0 && cam->baseline != 0.0, "voxel_map_carve: focal and baseline must not be 0");
  return SVO_OK;
}

inline int voxel_render_check(int width, int height, const svo_camera_info* cam, const double* w2c12, const svo_voxel_render_params* prm,
                              int max_width, int max_height, const char** err) {
  VOXEL_REFUSE(cam, "voxel_map_render: null cam");
  VOXEL_REFUSE(w2c12, "voxel_map_render: null w2c12");
  VOXEL_REFUSE(prm, "voxel_map_render: null params");
  VOXEL_REFUSE(prm->min_count >= 1, "voxel_map_render: min_count must be at least 1");
  VOXEL_REFUSE(prm->max_radius >= 0 && prm->max_radius <= 16, "voxel_map_render: max_radius outside 0..16");
  VOXEL_REFUSE(width >= 1 && width <= max_width, "voxel_map_render: width below 1 or beyond the context's limit");
  VOXEL_REFUSE(height >= 1 && height <= max_height, "voxel_map_render: height below 1 or beyond the context's limit");
  VOXEL_REFUSE(cam->focal > 0.0 && cam->focal <= DBL_MAX, "voxel_map_render: focal must be finite and > 0");  // a NaN fails the first test
  VOXEL_REFUSE(cam->baseline > 0.0 && cam->baseline <= DBL_MAX, "voxel_map_render: baseline must be finite and > 0");
  return SVO_OK;
}

// ----------------------------------------------------------------------------- the copy's box (lo_xyz, hi_xyz in map units) -> inclusive key range
inline int voxel_box_keys(const double* box6, float voxel_size, int klo[3], int khi[3], const char** err) {
  const double vs = (double)voxel_size, far = 2097152.0;  // 2^21: beyond every key on either side
  for (int i = 0; i < 6; ++i) {
    VOXEL_REFUSE(box6[i] == box6[i], "voxel_map_copy_live: box6 holds a NaN");
    double k = floor(box6[i] / vs);
    k = k < -far ? -far : (k > far ? far : k);
    (i < 3 ? klo[i] : khi[i - 3]) = (int)k;
  }
  return SVO_OK;
}

// ----------------------------------------------------------------------------- the grid (include/svo.h, "Voxel map grid")
inline int voxel_grid_params_check(const svo_voxel_grid_params* p, const char** err) {
  VOXEL_REFUSE(p, "voxel_map_grid: null params");
  VOXEL_REFUSE(p->up_axis >= 0 && p->up_axis <= 2, "voxel_map_grid: up_axis outside 0..2");
  VOXEL_REFUSE(p->up_sign == 1 || p->up_sign == -1, "voxel_map_grid: up_sign must be +1 or -1");
  VOXEL_REFUSE(p->origin_a >= -DBL_MAX && p->origin_a <= DBL_MAX, "voxel_map_grid: origin_a must be finite");  // a NaN fails the first test
  VOXEL_REFUSE(p->origin_b >= -DBL_MAX && p->origin_b <= DBL_MAX, "voxel_map_grid: origin_b must be finite");
  VOXEL_REFUSE(p->cell_voxels >= 1 && p->cell_voxels <= 1024, "voxel_map_grid: cell_voxels outside 1..1024");
  VOXEL_REFUSE(p->na >= 1 && p->na <= 8192, "voxel_map_grid: na outside 1..8192");
  VOXEL_REFUSE(p->nb >= 1 && p->nb <= 8192, "voxel_map_grid: nb outside 1..8192");
  VOXEL_REFUSE((long long)p->na * p->nb <= (1ll << 24), "voxel_map_grid: na * nb beyond 2^24");
  VOXEL_REFUSE(p->up_lo == p->up_lo && p->up_hi == p->up_hi, "voxel_map_grid: up_lo or up_hi is a NaN");
  VOXEL_REFUSE(p->up_lo <= p->up_hi, "voxel_map_grid: up_lo above up_hi");
  VOXEL_REFUSE(p->obstacle_step >= 0.0, "voxel_map_grid: obstacle_step must not be negative or a NaN");
  VOXEL_REFUSE(p->min_count >= 1, "voxel_map_grid: min_count must be at least 1");
  return SVO_OK;
}

// device: the _dev entry's pointers, whose alignment the kernels rely on; the synchronous entry copies into host pointers of any alignment.
inline int voxel_grid_out_check(const svo_voxel_grid_out* o, bool device, const char** err) {
  VOXEL_REFUSE(o, "voxel_map_grid: null out");
  VOXEL_REFUSE(o->cls, "voxel_map_grid: null cls");
  if (!device) return SVO_OK;
  VOXEL_REFUSE(((uintptr_t)o->top & 3u) == 0, "voxel_map_grid: top must be 4-byte aligned");
  VOXEL_REFUSE(((uintptr_t)o->bottom & 3u) == 0, "voxel_map_grid: bottom must be 4-byte aligned");
  VOXEL_REFUSE(((uintptr_t)o->n_voxels & 3u) == 0, "voxel_map_grid: n_voxels must be 4-byte aligned");
  VOXEL_REFUSE(((uintptr_t)o->n_points & 7u) == 0, "voxel_map_grid: n_points must be 8-byte aligned");
  return SVO_OK;
}

inline int voxel_grid_check(const svo_voxel_grid_params* p, const void* workspace, const svo_voxel_grid_out* o, const void* counts, const char** err) {
  if (const int rc = voxel_grid_params_check(p, err)) return rc;
  VOXEL_REFUSE(workspace, "voxel_map_grid: null workspace");
  VOXEL_REFUSE(((uintptr_t)workspace & 7u) == 0, "voxel_map_grid: workspace must be 8-byte aligned");
  if (const int rc = voxel_grid_out_check(o, true, err)) return rc;
  VOXEL_REFUSE(((uintptr_t)counts & 7u) == 0, "voxel_map_grid: counts must be 8-byte aligned");
  return SVO_OK;
}

inline size_t voxel_grid_workspace_bytes(int na, int nb) { return na < 1 || nb < 1 ? 0 : 32 * (size_t)na * (size_t)nb; }

// What the kernels take instead of the doubles: the origin's key indices, the band and the step in 65536ths of a voxel.
struct VoxelGridKeys {
  int ka0, kb0;
  long long hlo, hhi, step;
};

inline double voxel_grid_clamp(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }  // v is never a NaN here

inline int voxel_grid_index(double x, double vs) { return (int)voxel_grid_clamp(floor(x / vs), -2097152.0, 2097152.0); }  // +-2^21, as voxel_box_keys

inline long long voxel_grid_height(double h, double vs, double lo) {  // +-2^38: beyond every |hgt| < 2^37 on either side
  return (long long)voxel_grid_clamp(floor(h / vs * 65536.0), lo, 274877906944.0);
}

inline void voxel_grid_keys(const svo_voxel_grid_params* p, float voxel_size, VoxelGridKeys* k) {  // p has passed voxel_grid_params_check
  const double vs = (double)voxel_size;
  k->ka0 = voxel_grid_index(p->origin_a, vs);
  k->kb0 = voxel_grid_index(p->origin_b, vs);
  k->hlo = voxel_grid_height(p->up_lo, vs, -274877906944.0);
  k->hhi = voxel_grid_height(p->up_hi, vs, -274877906944.0);
  k->step = voxel_grid_height(p->obstacle_step, vs, 0.0);
}

// The floor of d / c for c >= 1, where C++ truncates.
#if defined(__HIPCC__)
#define VOXEL_HD __host__ __device__
#else
#define VOXEL_HD
#endif
VOXEL_HD inline int voxel_floordiv(int d, int c) {
  const int q = d / c;
  return q - ((d - q * c) < 0 ? 1 : 0);
}

// floor(s / c) for every s < 2^40 and 1 <= c < 2^24, without a 64-bit (or f64) division.  The loop keeps s = q c + r with r >= 0 and
// ends with r < c, so the result is exact whenever no step takes more than r / c off.  c is exact in f32 and r is off by at most
// 2^-24 of itself, so (float)r / (float)c scaled by 1 - 2^-18 never exceeds r / c (three roundings of 2^-24 each, and slack for a
// division a few ulp off) and falls short of it by less than 2^-17 of it; an estimate of 0 is 1, which r >= c allows.  The first
// step leaves r / c < 2^-17 s / c + 1: for the quotients a table of inserts holds (<= 65535) that is below 1.5, and the loop runs
// once or twice; for any s < 2^40 it runs at most five times.
VOXEL_HD inline unsigned long long voxel_div40(unsigned long long s, unsigned c) {
  const float cf = (float)c;
  unsigned long long q = 0, r = s;
  while (r >= (unsigned long long)c) {
    unsigned long long e = (unsigned long long)((float)r / cf * 0.999996185302734375f);  // 1 - 2^-18
    e = e ? e : 1ull;
    q += e;
    r -= e * (unsigned long long)c;
  }
  return q;
}

inline int voxel_grid_default_params(float voxel_size, svo_voxel_grid_params* p) {
  if (!p || !(voxel_size > 0.0f && voxel_size <= FLT_MAX)) return SVO_ERR_INVALID;
  const double vs = (double)voxel_size;
  p->up_axis = 1; p->up_sign = -1;  // the first camera's frame: y down
  p->cell_voxels = (int)voxel_grid_clamp(floor(0.5 / vs + 0.5), 1.0, 1024.0);
  p->na = 256; p->nb = 256;
  p->origin_a = 0.0; p->origin_b = -128.0 * (double)p->cell_voxels * vs;
  p->up_lo = -3.0; p->up_hi = 2.5;
  p->obstacle_step = 0.3;
  p->min_count = 1;
  return SVO_OK;
}

// 1: inside, 0: outside (ia, ib written all the same; either may be null), SVO_ERR_INVALID: refused.
inline int voxel_grid_cell_of(const svo_voxel_grid_params* p, float voxel_size, double a, double b, int* ia, int* ib) {
  const char* err = nullptr;
  if (voxel_grid_params_check(p, &err)) return SVO_ERR_INVALID;
  if (!(voxel_size > 0.0f && voxel_size <= FLT_MAX) || a != a || b != b) return SVO_ERR_INVALID;
  VoxelGridKeys k;
  voxel_grid_keys(p, voxel_size, &k);
  const double vs = (double)voxel_size;
  const int i = voxel_floordiv(voxel_grid_index(a, vs) - k.ka0, p->cell_voxels), j = voxel_floordiv(voxel_grid_index(b, vs) - k.kb0, p->cell_voxels);
  if (ia) *ia = i;
  if (ib) *ib = j;
  return i >= 0 && i < p->na && j >= 0 && j < p->nb ? 1 : 0;
}

// ----------------------------------------------------------------------------- launch geometry, in workgroups of VOXEL_THREADS
inline size_t voxel_div_up(size_t a, size_t b) { return (a + b - 1) / b; }
inline size_t voxel_walk_groups(size_t cap) { return voxel_div_up(cap, (size_t)VOXEL_THREADS * VOXEL_WALK_ITEMS); }
inline size_t voxel_record_groups(int n) { return voxel_div_up((size_t)n, VOXEL_THREADS); }
inline size_t voxel_resolve_groups(size_t pixels) { return voxel_div_up(pixels, (size_t)VOXEL_THREADS * VOXEL_RESOLVE_PIXELS); }
inline size_t voxel_grid_resolve_groups(size_t cells) { return voxel_div_up(cells, VOXEL_THREADS); }  // the grid's resolve: one cell per thread
// The resolve's vector form: a 16-byte load of the workspace, an 8-byte store of the map, a 4-byte store of the image (null: none).
inline bool voxel_resolve_vector_ok(const void* workspace, const void* disp16, const void* intensity) {
  return ((uintptr_t)workspace & 15u) == 0 && ((uintptr_t)disp16 & 7u) == 0 && ((uintptr_t)intensity & 3u) == 0;
}

#endif  // SVO_VOXEL_ARGS_H_
