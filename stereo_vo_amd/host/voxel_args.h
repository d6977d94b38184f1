// The voxel map's host logic that needs no GPU (include/svo.h, "voxel map"): the parameter test and the table's
// size, pose7 -> the two 3 x 4 matrices, the argument checks of the cloud, carve and render entries, the copy's box -> key range,
// and the launch geometry.  A refusal is SVO_ERR_INVALID with *err set to the message; csrc/voxel.hip stores it in the context
// and keeps no second copy of anything here.  tests/sanitize/voxel_args_test.cpp walks every refusal at its boundary on a CPU.
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

// ----------------------------------------------------------------------------- launch geometry, in workgroups of VOXEL_THREADS
inline size_t voxel_div_up(size_t a, size_t b) { return (a + b - 1) / b; }
inline size_t voxel_walk_groups(size_t cap) { return voxel_div_up(cap, (size_t)VOXEL_THREADS * VOXEL_WALK_ITEMS); }
inline size_t voxel_record_groups(int n) { return voxel_div_up((size_t)n, VOXEL_THREADS); }
inline size_t voxel_resolve_groups(size_t pixels) { return voxel_div_up(pixels, (size_t)VOXEL_THREADS * VOXEL_RESOLVE_PIXELS); }
// The resolve's vector form: a 16-byte load of the workspace, an 8-byte store of the map, a 4-byte store of the image (null: none).
inline bool voxel_resolve_vector_ok(const void* workspace, const void* disp16, const void* intensity) {
  return ((uintptr_t)workspace & 15u) == 0 && ((uintptr_t)disp16 & 7u) == 0 && ((uintptr_t)intensity & 3u) == 0;
}

#endif  // SVO_VOXEL_ARGS_H_
