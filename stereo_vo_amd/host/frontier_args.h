// The ground plan frontiers' host logic that needs no GPU (include/svo.h, "Ground plan frontiers"): the parameter and
// pointer checks with their message texts and their order, the workspace's layout and size, the launch geometry (tiles, seam cells,
// scan blocks) and the defaults.  A refusal is SVO_ERR_INVALID with *err set to the message; csrc/frontier.hip stores it in the
// context and keeps no second copy of anything here.  tests/sanitize/grid_frontier_args_test.cpp walks every refusal at its boundary
// on a CPU.
#ifndef SVO_FRONTIER_ARGS_H_
#define SVO_FRONTIER_ARGS_H_
#include <stddef.h>
#include <stdint.h>

#include "svo.h"

#define FRONTIER_REFUSE(cond, msg) do { if (!(cond)) { *err = (msg); return SVO_ERR_INVALID; } } while (0)

constexpr int FRONTIER_THREADS = 256;            // every kernel's workgroup
constexpr int FRONTIER_TILE = 16;                // T: the tile kernel's workgroup labels one T x T tile, a cell per thread
constexpr uint32_t FRONTIER_NONE = 0xFFFFFFFFu;
constexpr int FRONTIER_MAX_SIDE = 8192, FRONTIER_MAX_FRONTIERS = 65536;
constexpr long long FRONTIER_MAX_CELLS = 1ll << 24;
constexpr uint32_t FRONTIER_MAX_MIN_SIZE = 1u << 24;
constexpr size_t FRONTIER_HEADER_BYTES = 256;    // the workspace's first bytes: word 0 is n_kept, the rest is not used
constexpr size_t FRONTIER_SLOT_BYTES = 64;       // one frontier's running statistics (FrontierSlot of csrc/frontier.hip)
static_assert(FRONTIER_TILE * FRONTIER_TILE == FRONTIER_THREADS, "a cell per thread");

inline bool frontier_shape_ok(int na, int nb) {
  return na >= 1 && na <= FRONTIER_MAX_SIDE && nb >= 1 && nb <= FRONTIER_MAX_SIDE && (long long)na * nb <= FRONTIER_MAX_CELLS;
}

inline int frontier_params_check(const svo_grid_frontier_params* p, const char** err) {
  FRONTIER_REFUSE(p->na >= 1 && p->na <= FRONTIER_MAX_SIDE, "grid_frontier: na outside 1..8192");
  FRONTIER_REFUSE(p->nb >= 1 && p->nb <= FRONTIER_MAX_SIDE, "grid_frontier: nb outside 1..8192");
  FRONTIER_REFUSE((long long)p->na * p->nb <= FRONTIER_MAX_CELLS, "grid_frontier: na * nb beyond 2^24");
  FRONTIER_REFUSE(p->free_mask != 0u, "grid_frontier: free_mask is 0");
  FRONTIER_REFUSE(p->unknown_mask != 0u, "grid_frontier: unknown_mask is 0");
  FRONTIER_REFUSE(p->min_size >= 1u && p->min_size <= FRONTIER_MAX_MIN_SIZE, "grid_frontier: min_size outside 1..2^24");
  FRONTIER_REFUSE(p->max_frontiers >= 1 && p->max_frontiers <= FRONTIER_MAX_FRONTIERS, "grid_frontier: max_frontiers outside 1..65536");
  FRONTIER_REFUSE((p->free_mask & p->unknown_mask) == 0u, "grid_frontier: free_mask and unknown_mask share a bit");
  return SVO_OK;
}

// The order of the refusals: the nulls (cls, params, workspace, out), every range in the order of the fields, the masks' common
// bit, the three outputs all NULL, then the 4-byte alignments (cost, label, goal_cells) and the 8-byte ones (frontiers, workspace,
// counts).  device: the _dev entry, which has a workspace and whose pointers the kernels rely on; the synchronous entry takes host
// pointers of any alignment and no workspace.
inline int frontier_check(const void* cls, const void* cost, const svo_grid_frontier_params* p, const void* workspace,
                          const svo_grid_frontier_out* o, const void* counts, bool device, const char** err) {
  FRONTIER_REFUSE(cls, "grid_frontier: null cls");
  FRONTIER_REFUSE(p, "grid_frontier: null params");
  FRONTIER_REFUSE(!device || workspace, "grid_frontier: null workspace");
  FRONTIER_REFUSE(o, "grid_frontier: null out");
  if (const int rc = frontier_params_check(p, err)) return rc;
  FRONTIER_REFUSE(o->frontiers || o->goal_cells || o->label, "grid_frontier: frontiers, goal_cells and label are all null");
  if (!device) return SVO_OK;
  FRONTIER_REFUSE(((uintptr_t)cost & 3u) == 0, "grid_frontier: cost must be 4-byte aligned");
  FRONTIER_REFUSE(((uintptr_t)o->label & 3u) == 0, "grid_frontier: label must be 4-byte aligned");
  FRONTIER_REFUSE(((uintptr_t)o->goal_cells & 3u) == 0, "grid_frontier: goal_cells must be 4-byte aligned");
  FRONTIER_REFUSE(((uintptr_t)o->frontiers & 7u) == 0, "grid_frontier: frontiers must be 8-byte aligned");
  FRONTIER_REFUSE(((uintptr_t)workspace & 7u) == 0, "grid_frontier: workspace must be 8-byte aligned");
  FRONTIER_REFUSE(((uintptr_t)counts & 7u) == 0, "grid_frontier: counts must be 8-byte aligned");
  return SVO_OK;
}

// ----------------------------------------------------------------------------- tiles and launch geometry
inline size_t frontier_tiles_along(int cells) { return cells < 1 ? 0 : ((size_t)cells + FRONTIER_TILE - 1) / FRONTIER_TILE; }
inline size_t frontier_tiles(int na, int nb) { return frontier_tiles_along(na) * frontier_tiles_along(nb); }  // the tile kernel's workgroups
inline size_t frontier_groups(size_t items) { return (items + FRONTIER_THREADS - 1) / FRONTIER_THREADS; }  // one item per thread
// The seam kernel's threads: first the cells of the columns ib = T, 2T, ... (the far side of a seam between tile columns), column by
// column and ia ascending, then the cells of the rows ia = T, 2T, ..., row by row and ib ascending.  Each unites with its three
// neighbours on the near side, so a tile corner is seen from both lists and reaches the three other tiles.
inline size_t frontier_seam_cols(int na, int nb) { return na < 1 || nb < 1 ? 0 : (frontier_tiles_along(nb) - 1) * (size_t)na; }
inline size_t frontier_seam_rows(int na, int nb) { return na < 1 || nb < 1 ? 0 : (frontier_tiles_along(na) - 1) * (size_t)nb; }
inline size_t frontier_seam_cells(int na, int nb) { return frontier_seam_cols(na, nb) + frontier_seam_rows(na, nb); }
// The rank's blocks: FRONTIER_THREADS cells each; one workgroup scans their counts in a loop (at most 65,536 of them).
inline size_t frontier_scan_blocks(int na, int nb) { return na < 1 || nb < 1 ? 0 : frontier_groups((size_t)na * (size_t)nb); }

// The workspace: FRONTIER_HEADER_BYTES | max_frontiers slots of FRONTIER_SLOT_BYTES | one u32 per scan block, rounded up to 8 bytes |
// parent, one u32 per cell | size, one u32 per cell | rank, one u32 per cell; the whole rounded up to 8 bytes:
//   256 + 64 * max_frontiers + round8(4 * ceil(na * nb / 256)) + round8(12 * na * nb).
inline size_t frontier_round8(size_t b) { return (b + 7) & ~(size_t)7; }
inline size_t frontier_ws_slots_offset() { return FRONTIER_HEADER_BYTES; }
inline size_t frontier_ws_blocks_offset(int max_frontiers) { return FRONTIER_HEADER_BYTES + FRONTIER_SLOT_BYTES * (size_t)max_frontiers; }
inline size_t frontier_ws_cells_offset(int which, int na, int nb, int max_frontiers) {  // which: 0 parent, 1 size, 2 rank, 3 the end
  return frontier_ws_blocks_offset(max_frontiers) + frontier_round8(4 * frontier_scan_blocks(na, nb)) + 4 * (size_t)which * (size_t)na * (size_t)nb;
}
inline size_t frontier_workspace_bytes(int na, int nb, int max_frontiers) {
  if (!frontier_shape_ok(na, nb) || max_frontiers < 1 || max_frontiers > FRONTIER_MAX_FRONTIERS) return 0;
  return frontier_round8(frontier_ws_cells_offset(3, na, nb, max_frontiers));
}

// The defaults for the grid of a clearance: LEVEL cells are free, UNKNOWN cells unknown, frontiers of 3 cells and more, 1024 records.
inline int frontier_default_params(const svo_grid_clearance_params* c, svo_grid_frontier_params* p) {
  if (!c || !p) return SVO_ERR_INVALID;
  if (!frontier_shape_ok(c->na, c->nb)) return SVO_ERR_INVALID;
  p->na = c->na; p->nb = c->nb;
  p->free_mask = 1u << SVO_VOXEL_GRID_LEVEL;
  p->unknown_mask = 1u << SVO_VOXEL_GRID_UNKNOWN;
  p->min_size = 3;
  p->max_frontiers = 1024;
  return SVO_OK;
}
#endif  // SVO_FRONTIER_ARGS_H_
