// The voxel map route's logic that needs no GPU (include/svo.h, "Voxel map route"): the argument checks with their
// message texts and their order, the workspace's layout and size, the tile counts, the launch geometry, the defaults, and - as
// __host__ __device__ inline code, so that the kernels and a CPU program run the same statements - a neighbour code's offsets and
// weight, the 27 passable flags around a cell of a bit volume, the allowed moves they leave, a step's unit, the tile faces a cell
// touches, one cell's relaxation and rule 5 for one cell.  Integers only.  A refusal is SVO_ERR_INVALID with *err set to the message;
// csrc/voxel_route.hip stores it in the context and keeps no second copy of anything here.
// tests/sanitize/voxel_route_args_test.cpp walks all of it on a CPU.
#ifndef SVO_VOXEL_ROUTE_H_
#define SVO_VOXEL_ROUTE_H_
#include "voxel_distance.h"

constexpr int VOXEL_ROUTE_THREADS = 256;  // every kernel's workgroup
// A round's workgroup relaxes one TX x TY x TZ tile, two cells per thread.  Axis 0 is the contiguous one.  The kept shape is the
// long one; the cube (-DSVO_EXP_VOXEL_ROUTE_CUBE, a developer's build, never a product's) is the one it was measured against
// (DESIGN §7v).
#ifdef SVO_EXP_VOXEL_ROUTE_CUBE
constexpr int VOXEL_ROUTE_TX = 8, VOXEL_ROUTE_TY = 8, VOXEL_ROUTE_TZ = 8;
#else
constexpr int VOXEL_ROUTE_TX = 16, VOXEL_ROUTE_TY = 8, VOXEL_ROUTE_TZ = 4;
#endif
constexpr int VOXEL_ROUTE_MAX_SWEEPS = 64;  // sweeps of a tile in LDS per round; a tile that needs more marks itself active
constexpr uint32_t VOXEL_ROUTE_NONE = 0xFFFFFFFFu;  // SVO_VOXEL_ROUTE_NONE
constexpr int VOXEL_ROUTE_MAX_ROUNDS = 4096, VOXEL_ROUTE_MAX_GOALS = 65536, VOXEL_ROUTE_MAX_STARTS = 4096, VOXEL_ROUTE_MAX_PATH = 1 << 20;
constexpr uint32_t VOXEL_ROUTE_MAX_NEAR_R2 = 254u * 254u, VOXEL_ROUTE_MAX_PENALTY = 1u << 20, VOXEL_ROUTE_MAX_COST = 0x7F000000u;
constexpr size_t VOXEL_ROUTE_HEADER_WORDS = 16;  // the workspace's first words: the verdict, the parity and the tallies of csrc/voxel_route.hip
constexpr int VOXEL_ROUTE_SELF = 13, VOXEL_ROUTE_NO_MOVE = 255;  // next at a used goal; next where cost is NONE
constexpr int VOXEL_ROUTE_DEFAULT_ROUNDS = 32;  // the CPU trial of DESIGN §7v
enum { VOXEL_ROUTE_OK = 0, VOXEL_ROUTE_TRUNCATED = 1, VOXEL_ROUTE_UNREACHED = 2, VOXEL_ROUTE_OUT_OF_VOLUME = 3, VOXEL_ROUTE_NOT_CONVERGED = 4 };

// ----------------------------------------------------------------------------- the checks, in the contract's order
inline int voxel_route_params_check(const svo_voxel_route_params* p, int n_starts, const char** err) {
  VOXEL_REFUSE(p, "voxel_route: null params");
  VOXEL_REFUSE(p->near_r2 <= VOXEL_ROUTE_MAX_NEAR_R2, "voxel_route: near_r2 beyond 254^2");
  VOXEL_REFUSE((uint64_t)p->near_weight * p->near_r2 <= VOXEL_ROUTE_MAX_PENALTY, "voxel_route: near_weight * near_r2 beyond 2^20");
  VOXEL_REFUSE(p->max_cost >= 1u && p->max_cost <= VOXEL_ROUTE_MAX_COST, "voxel_route: max_cost outside 1..0x7F000000");
  VOXEL_REFUSE(p->max_rounds >= 1 && p->max_rounds <= VOXEL_ROUTE_MAX_ROUNDS, "voxel_route: max_rounds outside 1..4096");
  VOXEL_REFUSE(n_starts <= 0 || (p->max_path >= 1 && p->max_path <= VOXEL_ROUTE_MAX_PATH), "voxel_route: max_path outside 1..2^20");
  VOXEL_REFUSE(p->resume == 0 || p->resume == 1, "voxel_route: resume must be 0 or 1");
  return SVO_OK;
}

inline int voxel_route_closed_check(const void* closed, const char** err) {
  VOXEL_REFUSE(closed, "voxel_route: null closed");
  VOXEL_REFUSE(((uintptr_t)closed & 7u) == 0, "voxel_route: closed must be 8-byte aligned");
  return SVO_OK;
}

inline int voxel_route_lists_check(const void* goals, int n_goals, const void* starts, int n_starts, const char** err) {
  VOXEL_REFUSE(goals, "voxel_route: null goals");
  VOXEL_REFUSE(n_goals >= 1 && n_goals <= VOXEL_ROUTE_MAX_GOALS, "voxel_route: n_goals outside 1..65536");
  VOXEL_REFUSE(n_starts >= 0 && n_starts <= VOXEL_ROUTE_MAX_STARTS, "voxel_route: n_starts outside 0..4096");
  VOXEL_REFUSE(starts || n_starts == 0, "voxel_route: null starts with n_starts > 0");
  VOXEL_REFUSE(!starts || n_starts > 0, "voxel_route: starts with n_starts == 0");
  return SVO_OK;
}

inline int voxel_route_out_check(const svo_voxel_route_out* o, int n_starts, const char** err) {
  VOXEL_REFUSE(o, "voxel_route: null out");
  VOXEL_REFUSE(o->cost, "voxel_route: null cost");
  const int n_path = (o->path ? 1 : 0) + (o->path_len ? 1 : 0) + (o->path_status ? 1 : 0);
  VOXEL_REFUSE(n_path == 0 || n_path == 3, "voxel_route: path, path_len and path_status go together");
  VOXEL_REFUSE(n_path == 0 || n_starts > 0, "voxel_route: path outputs with n_starts == 0");
  return SVO_OK;
}

// The _dev entry's, after the null map: params, dims, closed, goals and starts, workspace, out and cost, the paths' consistency,
// then the alignments the kernels rely on.
inline int voxel_route_check(const void* closed, const int* dims, const void* dist2, const svo_voxel_route_params* p, const void* goals, int n_goals,
                             const void* starts, int n_starts, const void* workspace, const svo_voxel_route_out* o, const void* counts, const char** err) {
  if (const int rc = voxel_route_params_check(p, n_starts, err)) return rc;
  if (const int rc = voxel_occupancy_dims_check(dims, err)) return rc;
  if (const int rc = voxel_route_closed_check(closed, err)) return rc;
  if (const int rc = voxel_route_lists_check(goals, n_goals, starts, n_starts, err)) return rc;
  VOXEL_REFUSE(workspace, "voxel_route: null workspace");
  if (const int rc = voxel_route_out_check(o, n_starts, err)) return rc;
  VOXEL_REFUSE(((uintptr_t)o->cost & 3u) == 0, "voxel_route: cost must be 4-byte aligned");
  VOXEL_REFUSE(((uintptr_t)goals & 3u) == 0, "voxel_route: goals must be 4-byte aligned");
  VOXEL_REFUSE(((uintptr_t)starts & 3u) == 0, "voxel_route: starts must be 4-byte aligned");
  VOXEL_REFUSE(((uintptr_t)o->path & 3u) == 0, "voxel_route: path must be 4-byte aligned");
  VOXEL_REFUSE(((uintptr_t)o->path_len & 3u) == 0, "voxel_route: path_len must be 4-byte aligned");
  VOXEL_REFUSE(((uintptr_t)dist2 & 1u) == 0, "voxel_route: dist2 must be 2-byte aligned");
  VOXEL_REFUSE(((uintptr_t)workspace & 7u) == 0, "voxel_route: workspace must be 8-byte aligned");
  VOXEL_REFUSE(((uintptr_t)counts & 7u) == 0, "voxel_route: counts must be 8-byte aligned");
  return SVO_OK;
}

// The host form's: closed and dist2 stay device pointers, everything else is a host array of any alignment; no workspace.
inline int voxel_route_host_check(const void* closed, const int* dims, const void* dist2, const svo_voxel_route_params* p, const void* goals, int n_goals,
                                  const void* starts, int n_starts, const svo_voxel_route_out* o, const char** err) {
  if (const int rc = voxel_route_params_check(p, n_starts, err)) return rc;
  VOXEL_REFUSE(p->resume == 0, "voxel_route: resume needs the _dev entry, whose workspace outlives the call");
  if (const int rc = voxel_occupancy_dims_check(dims, err)) return rc;
  if (const int rc = voxel_route_closed_check(closed, err)) return rc;
  if (const int rc = voxel_route_lists_check(goals, n_goals, starts, n_starts, err)) return rc;
  if (const int rc = voxel_route_out_check(o, n_starts, err)) return rc;
  VOXEL_REFUSE(((uintptr_t)dist2 & 1u) == 0, "voxel_route: dist2 must be 2-byte aligned");
  return SVO_OK;
}

// ----------------------------------------------------------------------------- tiles, workspace, launch geometry, defaults
inline size_t voxel_route_tiles_along(int cells, int edge) { return cells < 1 ? 0 : ((size_t)cells + (size_t)edge - 1) / (size_t)edge; }
struct VoxelRouteTiles {
  size_t n0, n1, n2, total;  // tiles along each axis; a round's workgroups
};
inline VoxelRouteTiles voxel_route_tiles(const int* dims) {
  VoxelRouteTiles t;
  t.n0 = voxel_route_tiles_along(dims[0], VOXEL_ROUTE_TX);
  t.n1 = voxel_route_tiles_along(dims[1], VOXEL_ROUTE_TY);
  t.n2 = voxel_route_tiles_along(dims[2], VOXEL_ROUTE_TZ);
  t.total = t.n0 * t.n1 * t.n2;
  return t;
}
inline size_t voxel_route_groups(size_t items) { return voxel_div_up(items, VOXEL_ROUTE_THREADS); }  // one item per thread

// The workspace: VOXEL_ROUTE_HEADER_WORDS u32 | activity array 0, one u32 per tile | activity array 1 | one u8 per cell (the
// directions the path launch walks when the caller asks for no `next`), rounded up to 8 bytes.  dims are checked.
inline size_t voxel_route_ws_activity_offset(int which, const int* dims) { return 4 * (VOXEL_ROUTE_HEADER_WORDS + (size_t)which * voxel_route_tiles(dims).total); }
inline size_t voxel_route_ws_next_offset(const int* dims) { return voxel_route_ws_activity_offset(2, dims); }
inline int voxel_route_workspace_bytes(const int* dims, size_t* bytes) {
  if (!bytes) return SVO_ERR_INVALID;
  *bytes = 0;
  const char* err = nullptr;
  if (voxel_occupancy_dims_check(dims, &err)) return SVO_ERR_INVALID;
  *bytes = (voxel_route_ws_next_offset(dims) + voxel_distance_cells(dims) + 7) & ~(size_t)7;
  return SVO_OK;
}

// No penalty, the largest cap, 32 rounds (the CPU trial of DESIGN §7v), paths of up to 4096 cells.  NOT tuned on real data.  The
// voxel size is taken for the day the defaults depend on it.
inline int voxel_route_default_params(float voxel_size, svo_voxel_route_params* p) {
  if (!p || !(voxel_size > 0.0f && voxel_size <= FLT_MAX)) return SVO_ERR_INVALID;
  p->near_r2 = 0; p->near_weight = 0;
  p->max_cost = VOXEL_ROUTE_MAX_COST;
  p->max_rounds = VOXEL_ROUTE_DEFAULT_ROUNDS;
  p->max_path = 4096;
  p->resume = 0;
  return SVO_OK;
}

// A world position's cell number by the distance field's rule 9 (host/voxel_distance.h's statements); SVO_ERR_INVALID for a
// rejected or outside position and for arguments the occupancy refuses.
inline int voxel_occupancy_cell_of(float voxel_size, const int* origin, const int* dims, const float* xyz, uint32_t* cell) {
  if (!cell || !xyz || !(voxel_size > 0.0f && voxel_size <= FLT_MAX)) return SVO_ERR_INVALID;
  const char* err = nullptr;
  if (voxel_occupancy_origin_check(origin, &err) || voxel_occupancy_dims_check(dims, &err)) return SVO_ERR_INVALID;
  size_t B = 0;
  if (voxel_distance_cell_of(xyz, voxel_size, origin, dims, &B) != VOXEL_SPHERE_FREE) return SVO_ERR_INVALID;
  *cell = (uint32_t)B;  // below 2^30
  return SVO_OK;
}

// ----------------------------------------------------------------------------- the per-cell statements
#ifdef __HIP_DEVICE_COMPILE__
#define VOXEL_ROUTE_UNROLL _Pragma("unroll")
#else
#define VOXEL_ROUTE_UNROLL
#endif

// Rule 2's code k = 9 (dj2 + 1) + 3 (dj1 + 1) + (dj0 + 1), 0..26; 13 is the cell itself.
VOXEL_HD inline int voxel_route_d0(int k) { return k % 3 - 1; }
VOXEL_HD inline int voxel_route_d1(int k) { return k / 3 % 3 - 1; }
VOXEL_HD inline int voxel_route_d2(int k) { return k / 9 - 1; }
VOXEL_HD inline int voxel_route_code(int d0, int d1, int d2) { return 9 * (d2 + 1) + 3 * (d1 + 1) + (d0 + 1); }
// 5 / 7 / 9 for 1 / 2 / 3 changed coordinates (k != 13)
VOXEL_HD inline uint32_t voxel_route_weight(int k) {
  const int changed = (voxel_route_d0(k) != 0) + (voxel_route_d1(k) != 0) + (voxel_route_d2(k) != 0);
  return (uint32_t)(3 + 2 * changed);
}

struct VoxelRouteVolume {
  const uint64_t* closed;  // the bit words
  const uint16_t* dist2;   // or null
  int d0, d1, d2;
  uint32_t near_r2, near_weight, max_cost;
};

VOXEL_HD inline bool voxel_route_closed_bit(const uint64_t* closed, size_t cell) { return (closed[cell >> 6] >> (cell & 63)) & 1u; }

// Rule 1 plus the chamfer's unit: what a move INTO the cell costs per unit of w.  NONE16 is far: it is below no near_r2.
VOXEL_HD inline uint32_t voxel_route_unit(const VoxelRouteVolume& g, size_t cell) {
  if (!g.dist2) return 16u;
  const uint32_t d = g.dist2[cell];
  return 16u + (d != VOXEL_DISTANCE_NONE16 && d < g.near_r2 ? g.near_weight * (g.near_r2 - d) : 0u);
}

// Bit k: the cell at k's offsets from (j0, j1, j2) is inside the volume and passable; bit 13 is the cell itself.  Axis 0 does not
// run on: a j0 outside [0, d0) is outside.
VOXEL_HD inline uint32_t voxel_route_open27(const VoxelRouteVolume& g, int j0, int j1, int j2) {
  uint32_t open = 0;
  for (int k = 0; k < 27; ++k) {
    const int u0 = j0 + voxel_route_d0(k), u1 = j1 + voxel_route_d1(k), u2 = j2 + voxel_route_d2(k);
    if (u0 < 0 || u0 >= g.d0 || u1 < 0 || u1 >= g.d1 || u2 < 0 || u2 >= g.d2) continue;
    const size_t u = (size_t)u0 + (size_t)g.d0 * ((size_t)u1 + (size_t)g.d1 * (size_t)u2);
    open |= voxel_route_closed_bit(g.closed, u) ? 0u : 1u << k;
  }
  return open;
}

// Rule 2: bit k is set iff every cell of the box spanned by the cell and its neighbour k is open - both ends, and the 2 cells an
// edge move or the 6 a vertex move passes between.  Nothing is allowed out of a closed cell.  With k a constant after unrolling,
// `need` is one.
VOXEL_HD inline uint32_t voxel_route_allowed(uint32_t open27) {
  uint32_t allowed = 0;
  VOXEL_ROUTE_UNROLL
  for (int k = 0; k < 27; ++k) {
    if (k == VOXEL_ROUTE_SELF) continue;
    const int d0 = voxel_route_d0(k), d1 = voxel_route_d1(k), d2 = voxel_route_d2(k);
    uint32_t need = 0;
    VOXEL_ROUTE_UNROLL
    for (int s = 0; s < 8; ++s) need |= 1u << voxel_route_code(s & 1 ? d0 : 0, s & 2 ? d1 : 0, s & 4 ? d2 : 0);
    allowed |= (open27 & need) == need ? 1u << k : 0u;
  }
  return allowed;
}

// Bit k: a cell at (l0, l1, l2) of a t0 x t1 x t2 tile lies in the one-cell halo of the tile's neighbour at k's offsets.
VOXEL_HD inline uint32_t voxel_route_faces(int l0, int l1, int l2, int t0, int t1, int t2) {
  uint32_t faces = 0;
  VOXEL_ROUTE_UNROLL
  for (int k = 0; k < 27; ++k) {
    if (k == VOXEL_ROUTE_SELF) continue;
    const int d0 = voxel_route_d0(k), d1 = voxel_route_d1(k), d2 = voxel_route_d2(k);
    const bool on = (d0 == 0 || l0 == (d0 < 0 ? 0 : t0 - 1)) && (d1 == 0 || l1 == (d1 < 0 ? 0 : t1 - 1)) && (d2 == 0 || l2 == (d2 < 0 ? 0 : t2 - 1));
    faces |= on ? 1u << k : 0u;
  }
  return faces;
}

// One cell's relaxation: the least of c and cost_at(k) + step_at(k) over the allowed moves whose end has a cost, within max_cost.
// A candidate is looked at only where cost_at(k) is a cost: at most 0x7F000000 + 2^24, so u32 arithmetic does not wrap.
template <class CostAt, class StepAt>
VOXEL_HD inline uint32_t voxel_route_relax(uint32_t c, uint32_t allowed, uint32_t max_cost, CostAt cost_at, StepAt step_at) {
  uint32_t b = c;
  VOXEL_ROUTE_UNROLL
  for (int k = 0; k < 27; ++k) {
    if (k == VOXEL_ROUTE_SELF) continue;
    const uint32_t cu = cost_at(k);
    const uint32_t cand = cu + step_at(k);
    const bool ok = ((allowed >> k) & 1u) != 0u && cu != VOXEL_ROUTE_NONE && cand <= max_cost;
    b = ok && cand < b ? cand : b;
  }
  return b;
}

// Rule 5 for the cell B = j0 + d0 (j1 + d1 j2) of a converged field.
VOXEL_HD inline uint8_t voxel_route_next_one(const VoxelRouteVolume& g, const uint32_t* cost, size_t B) {
  const uint32_t c = cost[B];
  if (c == 0u) return (uint8_t)VOXEL_ROUTE_SELF;
  if (c == VOXEL_ROUTE_NONE) return (uint8_t)VOXEL_ROUTE_NO_MOVE;
  const size_t rest = B / (size_t)g.d0;
  const int j0 = (int)(B - rest * (size_t)g.d0), j1 = (int)(rest % (size_t)g.d1), j2 = (int)(rest / (size_t)g.d1);
  const uint32_t allowed = voxel_route_allowed(voxel_route_open27(g, j0, j1, j2));
  for (int k = 0; k < 27; ++k) {  // upward: the smallest k
    if (!((allowed >> k) & 1u)) continue;
    const size_t u = (size_t)(j0 + voxel_route_d0(k)) + (size_t)g.d0 * ((size_t)(j1 + voxel_route_d1(k)) + (size_t)g.d1 * (size_t)(j2 + voxel_route_d2(k)));
    const uint32_t cu = cost[u];
    if (cu != VOXEL_ROUTE_NONE && cu + voxel_route_weight(k) * voxel_route_unit(g, u) == c) return (uint8_t)k;
  }
  return (uint8_t)VOXEL_ROUTE_NO_MOVE;  // not reached on a converged field
}

// One step of a path's walk: the cell `next` byte k leads to from v, or NONE where k is no move or leaves the volume.
VOXEL_HD inline uint32_t voxel_route_step(uint32_t v, unsigned k, int d0, int d1, int d2) {
  if (k >= 27u || k == (unsigned)VOXEL_ROUTE_SELF) return VOXEL_ROUTE_NONE;
  const uint32_t rest = v / (uint32_t)d0;
  const int u0 = (int)(v - rest * (uint32_t)d0) + voxel_route_d0((int)k), u1 = (int)(rest % (uint32_t)d1) + voxel_route_d1((int)k),
            u2 = (int)(rest / (uint32_t)d1) + voxel_route_d2((int)k);
  if (u0 < 0 || u0 >= d0 || u1 < 0 || u1 >= d1 || u2 < 0 || u2 >= d2) return VOXEL_ROUTE_NONE;
  return (uint32_t)u0 + (uint32_t)d0 * ((uint32_t)u1 + (uint32_t)d1 * (uint32_t)u2);
}

#endif  // SVO_VOXEL_ROUTE_H_
