// The ground plan view's host logic that needs no GPU (include/svo.h, "Ground plan view"): the parameter and pointer
// checks with their message texts and their order, the workspace's layout and size, the launch geometry (the window's bit planes in
// LDS, the targets of a view), the ring enumeration that hands targets to threads and the defaults.  A refusal is SVO_ERR_INVALID
// with *err set to the message; csrc/view.hip stores it in the context and keeps no second copy of anything here.
// tests/sanitize/grid_view_args_test.cpp walks every refusal at its boundary and the ring enumeration on a CPU.
#ifndef SVO_VIEW_ARGS_H_
#define SVO_VIEW_ARGS_H_
#include <stddef.h>
#include <stdint.h>

#include "svo.h"

#if defined(__HIPCC__)
#define VIEW_HD __host__ __device__
#else
#define VIEW_HD
#endif

#define VIEW_REFUSE(cond, msg) do { if (!(cond)) { *err = (msg); return SVO_ERR_INVALID; } } while (0)

constexpr int VIEW_THREADS = 256;                // the rank kernel's workgroup
constexpr int VIEW_CAST_THREADS = 1024;          // the cast kernel's: a view is one workgroup, and its walks wait on one look-up after
                                                 // another, so sixteen wavefronts a view hide what four cannot (measured)
constexpr uint32_t VIEW_NONE = 0xFFFFFFFFu;
constexpr uint32_t VIEW_MAX_SCORE = 0xFFFFFFFEu;
constexpr int VIEW_MAX_SIDE = 8192, VIEW_MAX_VIEWS = SVO_GRID_VIEW_MAX_VIEWS, VIEW_MAX_RANGE = 255;
constexpr long long VIEW_MAX_CELLS = 1ll << 24;
constexpr uint32_t VIEW_MAX_GAIN_WEIGHT = 65536u, VIEW_MAX_COST_DIV = 1u << 31;
constexpr size_t VIEW_HEADER_BYTES = 256;        // the workspace's first bytes: not used
constexpr size_t VIEW_SLOT_BYTES = 16;           // what the cast leaves the rank per view (ViewSlot of csrc/view.hip)
constexpr size_t VIEW_LDS_LIMIT = 65536;         // the cast kernel's dynamic LDS stays below it at every accepted max_range

inline bool view_shape_ok(int na, int nb) {
  return na >= 1 && na <= VIEW_MAX_SIDE && nb >= 1 && nb <= VIEW_MAX_SIDE && (long long)na * nb <= VIEW_MAX_CELLS;
}

inline int view_params_check(const svo_grid_view_params* p, const char** err) {
  VIEW_REFUSE(p->na >= 1 && p->na <= VIEW_MAX_SIDE, "grid_view: na outside 1..8192");
  VIEW_REFUSE(p->nb >= 1 && p->nb <= VIEW_MAX_SIDE, "grid_view: nb outside 1..8192");
  VIEW_REFUSE((long long)p->na * p->nb <= VIEW_MAX_CELLS, "grid_view: na * nb beyond 2^24");
  VIEW_REFUSE(p->opaque_mask != 0u, "grid_view: opaque_mask is 0");
  VIEW_REFUSE(p->gain_mask != 0u, "grid_view: gain_mask is 0");
  VIEW_REFUSE(p->max_range >= 1 && p->max_range <= VIEW_MAX_RANGE, "grid_view: max_range outside 1..255");
  VIEW_REFUSE(p->gain_weight >= 1u && p->gain_weight <= VIEW_MAX_GAIN_WEIGHT, "grid_view: gain_weight outside 1..65536");
  VIEW_REFUSE(p->cost_div >= 1u && p->cost_div <= VIEW_MAX_COST_DIV, "grid_view: cost_div outside 1..2^31");
  return SVO_OK;
}

// The order of the refusals: the nulls (cls, params, views, workspace, out), every range in the order of the fields, n_views, the four
// outputs all NULL, then the 4-byte alignments (views, cost, order, best, seen) and the 8-byte ones (records, workspace, counts).
// device: the _dev entry, which has a workspace and whose pointers the kernels rely on; the synchronous entry takes host pointers of
// any alignment and no workspace.
inline int view_check(const void* cls, const void* views, int n_views, const void* cost, const svo_grid_view_params* p,
                      const void* workspace, const svo_grid_view_out* o, const void* counts, bool device, const char** err) {
  VIEW_REFUSE(cls, "grid_view: null cls");
  VIEW_REFUSE(p, "grid_view: null params");
  VIEW_REFUSE(views, "grid_view: null views");
  VIEW_REFUSE(!device || workspace, "grid_view: null workspace");
  VIEW_REFUSE(o, "grid_view: null out");
  if (const int rc = view_params_check(p, err)) return rc;
  VIEW_REFUSE(n_views >= 1 && n_views <= VIEW_MAX_VIEWS, "grid_view: n_views outside 1..4096");
  VIEW_REFUSE(o->records || o->order || o->best || o->seen, "grid_view: records, order, best and seen are all null");
  if (!device) return SVO_OK;
  VIEW_REFUSE(((uintptr_t)views & 3u) == 0, "grid_view: views must be 4-byte aligned");
  VIEW_REFUSE(((uintptr_t)cost & 3u) == 0, "grid_view: cost must be 4-byte aligned");
  VIEW_REFUSE(((uintptr_t)o->order & 3u) == 0, "grid_view: order must be 4-byte aligned");
  VIEW_REFUSE(((uintptr_t)o->best & 3u) == 0, "grid_view: best must be 4-byte aligned");
  VIEW_REFUSE(((uintptr_t)o->seen & 3u) == 0, "grid_view: seen must be 4-byte aligned");
  VIEW_REFUSE(((uintptr_t)o->records & 7u) == 0, "grid_view: records must be 8-byte aligned");
  VIEW_REFUSE(((uintptr_t)workspace & 7u) == 0, "grid_view: workspace must be 8-byte aligned");
  VIEW_REFUSE(((uintptr_t)counts & 7u) == 0, "grid_view: counts must be 8-byte aligned");
  return SVO_OK;
}

// ----------------------------------------------------------------------------- the window and the targets of one view
// The cast kernel's workgroup stages the (2R + 1)^2 window of cls around its view as two bit planes, OPAQUE then GAIN, row by row,
// every row padded to whole u32 words: bit (R + db) of row (R + da).  At R = 255 that is 2 * 511 * 16 words = 65,408 bytes.
VIEW_HD inline int view_window_side(int max_range) { return 2 * max_range + 1; }
VIEW_HD inline int view_window_row_words(int max_range) { return (view_window_side(max_range) + 31) / 32; }
VIEW_HD inline int view_window_plane_words(int max_range) { return view_window_side(max_range) * view_window_row_words(max_range); }
inline size_t view_lds_bytes(int max_range) { return max_range < 1 ? 0 : 2 * sizeof(uint32_t) * (size_t)view_window_plane_words(max_range); }
// Target 0 is V; targets 1 .. 4R(R + 1) are the rings of Chebyshev radius 1, 2, ..., R in turn, 8n cells each.
VIEW_HD inline uint32_t view_targets(int max_range) { return 1u + 4u * (uint32_t)max_range * ((uint32_t)max_range + 1u); }
VIEW_HD inline uint32_t view_ring_first(int n) { return 1u + 4u * (uint32_t)n * ((uint32_t)n - 1u); }  // ring n's first target, n >= 1
// The ring of target g, 1 <= g < view_targets(255): the largest n with view_ring_first(n) <= g, by bisection in 8 steps.
VIEW_HD inline int view_ring_of(uint32_t g) {
  int lo = 1, hi = VIEW_MAX_RANGE;
  for (int step = 0; step < 8; ++step) {
    const int mid = (lo + hi + 1) >> 1;
    if (view_ring_first(mid) <= g) lo = mid; else hi = mid - 1;
  }
  return lo;
}
// Ring n, position k in 0..8n-1 -> (da, db), clockwise from the corner (-n, -n): the side da = -n with db rising, the side db = +n
// with da rising, the side da = +n with db falling, the side db = -n with da falling; 2n cells each, every corner once.
VIEW_HD inline void view_ring_cell(int n, int k, int* da, int* db) {
  const int side = k / (2 * n), t = k - side * 2 * n;
  if (side == 0) { *da = -n; *db = -n + t; }
  else if (side == 1) { *da = -n + t; *db = n; }
  else if (side == 2) { *da = n; *db = n - t; }
  else { *da = n - t; *db = -n; }
}
VIEW_HD inline void view_target_cell(uint32_t g, int* da, int* db) {
  if (g == 0u) { *da = 0; *db = 0; return; }
  const int n = view_ring_of(g);
  view_ring_cell(n, (int)(g - view_ring_first(n)), da, db);
}
// The cast kernel's loop: every thread takes targets tid, tid + VIEW_CAST_THREADS, ...; the same trip count for every thread.
inline uint32_t view_target_rounds(int max_range) { return (view_targets(max_range) + VIEW_CAST_THREADS - 1) / VIEW_CAST_THREADS; }

// Rule 6.  cost: the view's cell's cost (NONE: unreachable), has_cost: whether a cost field was given.
VIEW_HD inline uint32_t view_score(uint32_t n_gain, uint32_t cost, bool has_cost, uint32_t gain_weight, uint32_t cost_div) {
  if (has_cost && cost == VIEW_NONE) return 0u;
  const uint64_t g = (uint64_t)gain_weight * (uint64_t)n_gain, c = has_cost ? (uint64_t)(cost / cost_div) : 0u;
  if (g <= c) return 0u;
  return g - c > (uint64_t)VIEW_MAX_SCORE ? VIEW_MAX_SCORE : (uint32_t)(g - c);
}

// The workspace: VIEW_HEADER_BYTES | n_views slots of VIEW_SLOT_BYTES | one u32 per cell (seen's stand-in), rounded up to 8 bytes:
//   256 + 16 * n_views + round8(4 * na * nb).
inline size_t view_round8(size_t b) { return (b + 7) & ~(size_t)7; }
inline size_t view_ws_slots_offset() { return VIEW_HEADER_BYTES; }
inline size_t view_ws_seen_offset(int n_views) { return VIEW_HEADER_BYTES + VIEW_SLOT_BYTES * (size_t)n_views; }
inline size_t view_workspace_bytes(int na, int nb, int n_views) {
  if (!view_shape_ok(na, nb) || n_views < 1 || n_views > VIEW_MAX_VIEWS) return 0;
  return view_ws_seen_offset(n_views) + view_round8(4 * (size_t)na * (size_t)nb);
}

// The defaults for the grid of a clearance: OBSTACLE cells are opaque, UNKNOWN cells are the gain (looked through), the clearance's
// reach as the range, 16 per gained cell against the undivided cost.
inline int view_default_params(const svo_grid_clearance_params* c, svo_grid_view_params* p) {
  if (!c || !p) return SVO_ERR_INVALID;
  if (!view_shape_ok(c->na, c->nb)) return SVO_ERR_INVALID;
  p->na = c->na; p->nb = c->nb;
  p->opaque_mask = 1u << SVO_VOXEL_GRID_OBSTACLE;
  p->gain_mask = 1u << SVO_VOXEL_GRID_UNKNOWN;
  p->max_range = c->max_dist < 1 ? 1 : (c->max_dist > VIEW_MAX_RANGE ? VIEW_MAX_RANGE : c->max_dist);
  p->gain_weight = 16u;
  p->cost_div = 1u;
  return SVO_OK;
}
#endif  // SVO_VIEW_ARGS_H_
