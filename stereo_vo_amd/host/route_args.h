// The ground plan route's host logic that needs no GPU (include/svo.h, "Ground plan route"): the parameter and pointer
// checks with their message texts, the workspace's layout and size, the tile count, the launch geometry and the defaults.  A refusal
// is SVO_ERR_INVALID with *err set to the message; csrc/route.hip stores it in the context and keeps no second copy of anything
// here.  tests/sanitize/grid_route_args_test.cpp walks every refusal at its boundary on a CPU.
#ifndef SVO_ROUTE_ARGS_H_
#define SVO_ROUTE_ARGS_H_
#include <stddef.h>
#include <stdint.h>

#include "svo.h"

#define ROUTE_REFUSE(cond, msg) do { if (!(cond)) { *err = (msg); return SVO_ERR_INVALID; } } while (0)

constexpr int ROUTE_THREADS = 256;            // every kernel's workgroup
constexpr int ROUTE_TILE = 16;                // T: a round's workgroup relaxes one T x T tile, a cell per thread (measured against 32)
constexpr int ROUTE_MAX_SWEEPS = 4 * ROUTE_TILE;  // sweeps of a tile in LDS per round; a tile that needs more marks itself active
constexpr uint32_t ROUTE_NONE = 0xFFFFFFFFu;  // SVO_GRID_ROUTE_NONE
constexpr int ROUTE_MAX_SIDE = 8192, ROUTE_MAX_ROUNDS = 4096, ROUTE_MAX_GOALS = 65536, ROUTE_MAX_STARTS = 4096, ROUTE_MAX_PATH = 1 << 20;
constexpr long long ROUTE_MAX_CELLS = 1ll << 24;
constexpr uint32_t ROUTE_MAX_NEAR_R2 = 1u << 26, ROUTE_MAX_PENALTY = 1u << 20, ROUTE_MAX_COST = 0x7F000000u;
constexpr size_t ROUTE_HEADER_WORDS = 16;     // the workspace's first words: the verdict, the parity and the tallies of csrc/route.hip

inline int route_params_check(const svo_grid_route_params* p, int n_starts, const char** err) {
  ROUTE_REFUSE(p, "grid_route: null params");
  ROUTE_REFUSE(p->na >= 1 && p->na <= ROUTE_MAX_SIDE, "grid_route: na outside 1..8192");
  ROUTE_REFUSE(p->nb >= 1 && p->nb <= ROUTE_MAX_SIDE, "grid_route: nb outside 1..8192");
  ROUTE_REFUSE((long long)p->na * p->nb <= ROUTE_MAX_CELLS, "grid_route: na * nb beyond 2^24");
  ROUTE_REFUSE(p->near_r2 <= ROUTE_MAX_NEAR_R2, "grid_route: near_r2 beyond 2^26");
  ROUTE_REFUSE((uint64_t)p->near_weight * p->near_r2 <= ROUTE_MAX_PENALTY, "grid_route: near_weight * near_r2 beyond 2^20");
  ROUTE_REFUSE(p->max_cost >= 1u && p->max_cost <= ROUTE_MAX_COST, "grid_route: max_cost outside 1..0x7F000000");
  ROUTE_REFUSE(p->max_rounds >= 1 && p->max_rounds <= ROUTE_MAX_ROUNDS, "grid_route: max_rounds outside 1..4096");
  ROUTE_REFUSE(n_starts <= 0 || (p->max_path >= 1 && p->max_path <= ROUTE_MAX_PATH), "grid_route: max_path outside 1..2^20");
  ROUTE_REFUSE(p->resume == 0 || p->resume == 1, "grid_route: resume must be 0 or 1");
  return SVO_OK;
}

inline int route_lists_check(const void* goals, int n_goals, const void* starts, int n_starts, const char** err) {
  ROUTE_REFUSE(goals, "grid_route: null goals");
  ROUTE_REFUSE(n_goals >= 1 && n_goals <= ROUTE_MAX_GOALS, "grid_route: n_goals outside 1..65536");
  ROUTE_REFUSE(n_starts >= 0 && n_starts <= ROUTE_MAX_STARTS, "grid_route: n_starts outside 0..4096");
  ROUTE_REFUSE(starts || n_starts == 0, "grid_route: null starts with n_starts > 0");
  return SVO_OK;
}

// device: the _dev entry's pointers, whose alignment the kernels rely on; the synchronous entry copies into host pointers of any alignment.
inline int route_out_check(const svo_grid_route_out* o, int n_starts, bool device, const char** err) {
  ROUTE_REFUSE(o, "grid_route: null out");
  ROUTE_REFUSE(o->cost, "grid_route: null cost");
  const int n_path = (o->path ? 1 : 0) + (o->path_len ? 1 : 0) + (o->path_status ? 1 : 0);
  ROUTE_REFUSE(n_path == 0 || n_path == 3, "grid_route: path, path_len and path_status go together");
  ROUTE_REFUSE(n_path == 0 || n_starts > 0, "grid_route: path outputs with n_starts == 0");
  if (!device) return SVO_OK;
  ROUTE_REFUSE(((uintptr_t)o->cost & 3u) == 0, "grid_route: cost must be 4-byte aligned");
  ROUTE_REFUSE(((uintptr_t)o->path & 3u) == 0, "grid_route: path must be 4-byte aligned");
  ROUTE_REFUSE(((uintptr_t)o->path_len & 3u) == 0, "grid_route: path_len must be 4-byte aligned");
  return SVO_OK;
}

// The order of the refusals: blocked, params, goals and starts, workspace, out, then the alignments of the inputs and of counts.
inline int route_check(const void* blocked, const void* dist2, const svo_grid_route_params* p, const void* goals, int n_goals,
                       const void* starts, int n_starts, const void* workspace, const svo_grid_route_out* o, const void* counts,
                       const char** err) {
  ROUTE_REFUSE(blocked, "grid_route: null blocked");
  if (const int rc = route_params_check(p, n_starts, err)) return rc;
  if (const int rc = route_lists_check(goals, n_goals, starts, n_starts, err)) return rc;
  ROUTE_REFUSE(workspace, "grid_route: null workspace");
  if (const int rc = route_out_check(o, n_starts, true, err)) return rc;
  ROUTE_REFUSE(((uintptr_t)dist2 & 3u) == 0, "grid_route: dist2 must be 4-byte aligned");
  ROUTE_REFUSE(((uintptr_t)goals & 3u) == 0, "grid_route: goals must be 4-byte aligned");
  ROUTE_REFUSE(((uintptr_t)starts & 3u) == 0, "grid_route: starts must be 4-byte aligned");
  ROUTE_REFUSE(((uintptr_t)workspace & 7u) == 0, "grid_route: workspace must be 8-byte aligned");
  ROUTE_REFUSE(((uintptr_t)counts & 7u) == 0, "grid_route: counts must be 8-byte aligned");
  return SVO_OK;
}

// ----------------------------------------------------------------------------- tiles and launch geometry
inline size_t route_tiles_along(int cells) { return cells < 1 ? 0 : ((size_t)cells + ROUTE_TILE - 1) / ROUTE_TILE; }  // in size_t: no wrap at INT_MAX
inline size_t route_tiles(int na, int nb) { return route_tiles_along(na) * route_tiles_along(nb); }  // a round's workgroups
inline size_t route_groups(size_t items) { return (items + ROUTE_THREADS - 1) / ROUTE_THREADS; }  // one item per thread

// The workspace: ROUTE_HEADER_WORDS u32 | activity array 0, one u32 per tile | activity array 1 | one u8 per cell (the directions the
// path launch walks when the caller asks for no `next`), rounded up to 8 bytes.
inline size_t route_ws_activity_offset(int which, int na, int nb) { return 4 * (ROUTE_HEADER_WORDS + (size_t)which * route_tiles(na, nb)); }
inline size_t route_ws_next_offset(int na, int nb) { return route_ws_activity_offset(2, na, nb); }
inline size_t route_workspace_bytes(int na, int nb) {
  return na < 1 || nb < 1 ? 0 : (route_ws_next_offset(na, nb) + (size_t)na * (size_t)nb + 7) & ~(size_t)7;
}

// The defaults for the grid of a clearance: no penalty, the largest cap, 64 rounds, paths of up to 4096 cells.
inline int route_default_params(const svo_grid_clearance_params* c, svo_grid_route_params* p) {
  if (!c || !p) return SVO_ERR_INVALID;
  if (c->na < 1 || c->na > ROUTE_MAX_SIDE || c->nb < 1 || c->nb > ROUTE_MAX_SIDE || (long long)c->na * c->nb > ROUTE_MAX_CELLS) return SVO_ERR_INVALID;
  p->na = c->na; p->nb = c->nb;
  p->near_r2 = 0; p->near_weight = 0;
  p->max_cost = ROUTE_MAX_COST;
  p->max_rounds = 64;
  p->max_path = 4096;
  p->resume = 0;
  return SVO_OK;
}
#endif  // SVO_ROUTE_ARGS_H_
