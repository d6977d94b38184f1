// The ground plan clearance's host logic that needs no GPU (include/svo.h, "Ground plan clearance"): the parameter and
// pointer checks with their message texts, the disc's squared radius R2, the workspace size, the launch geometry and the defaults.
// A refusal is SVO_ERR_INVALID with *err set to the message; csrc/clearance.hip stores it in the context and keeps no second copy
// of anything here.  tests/sanitize/grid_clearance_args_test.cpp walks every refusal at its boundary on a CPU.
#ifndef SVO_CLEARANCE_ARGS_H_
#define SVO_CLEARANCE_ARGS_H_
#include <float.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "svo.h"

#define CLEARANCE_REFUSE(cond, msg) do { if (!(cond)) { *err = (msg); return SVO_ERR_INVALID; } } while (0)

constexpr int CLEARANCE_THREADS = 256;               // both kernels' workgroup: one cell per thread
constexpr uint32_t CLEARANCE_NONE = 0xFFFFFFFFu;     // SVO_GRID_CLEARANCE_NONE: dist2 and nearest of a cell no source reaches
constexpr int32_t CLEARANCE_NO_OFFSET = 0x7FFFFFFF;  // the workspace word of a cell with no source within max_dist in its row
constexpr int CLEARANCE_MAX_SIDE = 8192, CLEARANCE_MAX_DIST = 8191;
constexpr long long CLEARANCE_MAX_CELLS = 1ll << 24;

inline int clearance_params_check(const svo_grid_clearance_params* p, const char** err) {
  CLEARANCE_REFUSE(p, "grid_clearance: null params");
  CLEARANCE_REFUSE(p->na >= 1 && p->na <= CLEARANCE_MAX_SIDE, "grid_clearance: na outside 1..8192");
  CLEARANCE_REFUSE(p->nb >= 1 && p->nb <= CLEARANCE_MAX_SIDE, "grid_clearance: nb outside 1..8192");
  CLEARANCE_REFUSE((long long)p->na * p->nb <= CLEARANCE_MAX_CELLS, "grid_clearance: na * nb beyond 2^24");
  CLEARANCE_REFUSE(p->source_mask != 0u, "grid_clearance: source_mask must not be 0");
  CLEARANCE_REFUSE(p->max_dist >= 1 && p->max_dist <= CLEARANCE_MAX_DIST, "grid_clearance: max_dist outside 1..8191");
  CLEARANCE_REFUSE(p->cell_size > 0.0 && p->cell_size <= DBL_MAX, "grid_clearance: cell_size must be finite and > 0");  // a NaN fails the first test
  CLEARANCE_REFUSE(p->inflate_radius >= 0.0 && p->inflate_radius <= DBL_MAX, "grid_clearance: inflate_radius must be finite and >= 0");
  return SVO_OK;
}

// device: the _dev entry's pointers, whose alignment the kernels rely on; the synchronous entry copies into host pointers of any alignment.
inline int clearance_out_check(const svo_grid_clearance_out* o, bool device, const char** err) {
  CLEARANCE_REFUSE(o, "grid_clearance: null out");
  CLEARANCE_REFUSE(o->dist2, "grid_clearance: null dist2");
  if (!device) return SVO_OK;
  CLEARANCE_REFUSE(((uintptr_t)o->dist2 & 3u) == 0, "grid_clearance: dist2 must be 4-byte aligned");
  CLEARANCE_REFUSE(((uintptr_t)o->nearest & 3u) == 0, "grid_clearance: nearest must be 4-byte aligned");
  CLEARANCE_REFUSE(((uintptr_t)o->clearance & 3u) == 0, "grid_clearance: clearance must be 4-byte aligned");
  return SVO_OK;
}

inline int clearance_check(const void* cls, const svo_grid_clearance_params* p, const void* workspace, const svo_grid_clearance_out* o,
                           const void* counts, const char** err) {
  CLEARANCE_REFUSE(cls, "grid_clearance: null cls");
  if (const int rc = clearance_params_check(p, err)) return rc;
  CLEARANCE_REFUSE(workspace, "grid_clearance: null workspace");
  CLEARANCE_REFUSE(((uintptr_t)workspace & 3u) == 0, "grid_clearance: workspace must be 4-byte aligned");
  if (const int rc = clearance_out_check(o, true, err)) return rc;
  CLEARANCE_REFUSE(((uintptr_t)counts & 7u) == 0, "grid_clearance: counts must be 8-byte aligned");
  return SVO_OK;
}

inline size_t clearance_workspace_bytes(int na, int nb) { return na < 1 || nb < 1 ? 0 : 4 * (size_t)na * (size_t)nb; }

// Rule 5's R2 = floor(rc * rc) clamped to max_dist^2, rc = inflate_radius / cell_size: two stated f64 operations and a floor.  p has
// passed clearance_params_check, so nothing here is a NaN; a quotient or a square that overflows is +infinity and takes the clamp.
inline uint32_t clearance_r2(const svo_grid_clearance_params* p) {
  const double rc = p->inflate_radius / p->cell_size;
  const double q = floor(rc * rc), cap = (double)p->max_dist * (double)p->max_dist;  // at most 8191^2 < 2^26
  return (uint32_t)(q < cap ? q : cap);
}

// ----------------------------------------------------------------------------- launch geometry, in workgroups of CLEARANCE_THREADS
inline size_t clearance_groups(size_t cells) { return (cells + CLEARANCE_THREADS - 1) / CLEARANCE_THREADS; }

// The defaults for a grid of svo_voxel_map_grid*: its shape, its cell edge in map units, OBSTACLE cells as the sources, 64 cells.
inline int clearance_default_params(const svo_voxel_grid_params* g, float voxel_size, svo_grid_clearance_params* p) {
  if (!g || !p || !(voxel_size > 0.0f && voxel_size <= FLT_MAX)) return SVO_ERR_INVALID;
  if (g->cell_voxels < 1 || g->cell_voxels > 1024 || g->na < 1 || g->na > CLEARANCE_MAX_SIDE || g->nb < 1 || g->nb > CLEARANCE_MAX_SIDE ||
      (long long)g->na * g->nb > CLEARANCE_MAX_CELLS)
    return SVO_ERR_INVALID;
  p->na = g->na; p->nb = g->nb;
  p->source_mask = 1u << SVO_VOXEL_GRID_OBSTACLE;
  p->max_dist = 64;
  p->cell_size = (double)g->cell_voxels * (double)voxel_size;
  p->inflate_radius = 0.0;
  return SVO_OK;
}
#endif  // SVO_CLEARANCE_ARGS_H_
