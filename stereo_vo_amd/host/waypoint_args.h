// The ground plan waypoints' host logic that needs no GPU (include/svo.h, "Ground plan waypoints"): the parameter and
// pointer checks with their message texts and their order, rule 3's line stepper by remainders and rule 4's CLEAR over a look-up
// functor (one definition for the kernel and for host programs) and the defaults.  A refusal is SVO_ERR_INVALID with *err set to the message; csrc/waypoints.hip stores it in the context and keeps no second
// copy of anything here.  tests/sanitize/grid_waypoints_args_test.cpp walks every refusal at its boundary, the stepper against the
// closed formula and CLEAR on hand-made corners on a CPU.
#ifndef SVO_WAYPOINT_ARGS_H_
#define SVO_WAYPOINT_ARGS_H_
#include <float.h>
#include <stddef.h>
#include <stdint.h>

#include "svo.h"

#if defined(__HIPCC__)
#define WAY_HD __host__ __device__
#else
#define WAY_HD
#endif

#define WAY_REFUSE(cond, msg) do { if (!(cond)) { *err = (msg); return SVO_ERR_INVALID; } } while (0)

constexpr int WAY_THREADS = 256;  // one candidate per thread: max_look <= 255 candidates a waypoint (1,024 measured and dropped)
constexpr int WAY_MAX_SIDE = 8192, WAY_MAX_LOOK = 255, WAY_MAX_PATHS = SVO_GRID_WAY_MAX_PATHS;
constexpr int WAY_MAX_STRIDE = 1 << 20, WAY_MAX_WAY = 1 << 20;
constexpr long long WAY_MAX_CELLS = 1ll << 24;
constexpr uint32_t WAY_MAX_DIST2 = 1u << 26;

inline bool way_shape_ok(int na, int nb) {
  return na >= 1 && na <= WAY_MAX_SIDE && nb >= 1 && nb <= WAY_MAX_SIDE && (long long)na * nb <= WAY_MAX_CELLS;
}

inline int way_params_check(const svo_grid_waypoint_params* p, const char** err) {
  WAY_REFUSE(p->na >= 1 && p->na <= WAY_MAX_SIDE, "grid_waypoints: na outside 1..8192");
  WAY_REFUSE(p->nb >= 1 && p->nb <= WAY_MAX_SIDE, "grid_waypoints: nb outside 1..8192");
  WAY_REFUSE((long long)p->na * p->nb <= WAY_MAX_CELLS, "grid_waypoints: na * nb beyond 2^24");
  WAY_REFUSE(p->path_stride >= 1 && p->path_stride <= WAY_MAX_STRIDE, "grid_waypoints: path_stride outside 1..2^20");
  WAY_REFUSE(p->max_look >= 1 && p->max_look <= WAY_MAX_LOOK, "grid_waypoints: max_look outside 1..255");
  WAY_REFUSE(p->min_dist2 <= WAY_MAX_DIST2, "grid_waypoints: min_dist2 beyond 2^26");
  WAY_REFUSE(p->max_way >= 1 && p->max_way <= WAY_MAX_WAY, "grid_waypoints: max_way outside 1..2^20");
  WAY_REFUSE(p->cell_size > 0.0 && p->cell_size <= DBL_MAX, "grid_waypoints: cell_size must be finite and > 0");  // a NaN fails the first test
  return SVO_OK;
}

// The order of the refusals (rule 8): the nulls (blocked, params, path, path_len, out), every range in the order of the fields,
// n_paths, the outputs' rules (way and way_len together, not every output NULL), then the 4-byte alignments (dist2, path, path_len,
// way, way_index, way_len) and the 8-byte ones (length, counts).  device: the _dev entry, whose pointers the kernel relies on; the
// synchronous entry takes host pointers of any alignment.
inline int way_check(const void* blocked, const void* dist2, const void* path, const void* path_len, int n_paths,
                     const svo_grid_waypoint_params* p, const svo_grid_waypoint_out* o, const void* counts, bool device, const char** err) {
  WAY_REFUSE(blocked, "grid_waypoints: null blocked");
  WAY_REFUSE(p, "grid_waypoints: null params");
  WAY_REFUSE(path, "grid_waypoints: null path");
  WAY_REFUSE(path_len, "grid_waypoints: null path_len");
  WAY_REFUSE(o, "grid_waypoints: null out");
  if (const int rc = way_params_check(p, err)) return rc;
  WAY_REFUSE(n_paths >= 1 && n_paths <= WAY_MAX_PATHS, "grid_waypoints: n_paths outside 1..4096");
  WAY_REFUSE((o->way != nullptr) == (o->way_len != nullptr), "grid_waypoints: way and way_len go together");
  WAY_REFUSE(o->way || o->way_index || o->way_len || o->way_status || o->length, "grid_waypoints: every output is null");
  if (!device) return SVO_OK;
  WAY_REFUSE(((uintptr_t)dist2 & 3u) == 0, "grid_waypoints: dist2 must be 4-byte aligned");
  WAY_REFUSE(((uintptr_t)path & 3u) == 0, "grid_waypoints: path must be 4-byte aligned");
  WAY_REFUSE(((uintptr_t)path_len & 3u) == 0, "grid_waypoints: path_len must be 4-byte aligned");
  WAY_REFUSE(((uintptr_t)o->way & 3u) == 0, "grid_waypoints: way must be 4-byte aligned");
  WAY_REFUSE(((uintptr_t)o->way_index & 3u) == 0, "grid_waypoints: way_index must be 4-byte aligned");
  WAY_REFUSE(((uintptr_t)o->way_len & 3u) == 0, "grid_waypoints: way_len must be 4-byte aligned");
  WAY_REFUSE(((uintptr_t)o->length & 7u) == 0, "grid_waypoints: length must be 8-byte aligned");
  WAY_REFUSE(((uintptr_t)counts & 7u) == 0, "grid_waypoints: counts must be 8-byte aligned");
  return SVO_OK;
}

// ----------------------------------------------------------------------------- rule 3's line and rule 4's CLEAR
// The line from V by remainders: after i steps the offset from V is (sa * pa, sb * pb) with
//   pa = floor((2 i |da| + n) / (2n)), ra = (2 i |da| + n) mod 2n, and the same for b; n = max(|da|, |db|) >= 1.
struct WayLine {
  int ada, adb, sa, sb, n;
  int ra, rb, pa, pb;
};
WAY_HD inline WayLine way_line(int da, int db) {
  WayLine l;
  l.ada = da < 0 ? -da : da; l.adb = db < 0 ? -db : db; l.sa = da < 0 ? -1 : 1; l.sb = db < 0 ? -1 : 1;
  l.n = l.ada > l.adb ? l.ada : l.adb;
  l.ra = l.n; l.rb = l.n; l.pa = 0; l.pb = 0;  // L_0 = V
  return l;
}
// L_(i-1) -> L_i, to be called at most n times.
WAY_HD inline void way_line_step(WayLine* l) {
  l->ra += 2 * l->ada; if (l->ra >= 2 * l->n) { l->ra -= 2 * l->n; ++l->pa; }
  l->rb += 2 * l->adb; if (l->rb >= 2 * l->n) { l->rb -= 2 * l->n; ++l->pb; }
}

// Rule 4.  solid(ia, ib) is asked only for cells in the bounding box of V and T, both of which the caller knows to be inside the grid.
template <class Solid>
WAY_HD inline bool way_clear(int va, int vb, int ta, int tb, int max_look, const Solid& solid) {
  WayLine l = way_line(ta - va, tb - vb);
  if (l.n > max_look) return false;
  if (solid(va, vb)) return false;
  if (l.n == 0) return true;
  if (solid(ta, tb)) return false;
  for (int i = 1; i <= l.n; ++i) {  // n <= 255
    const int qa = l.pa, qb = l.pb;
    way_line_step(&l);
    // The three look-ups of a step are asked for together and combined without branches between them; where the step is along an
    // axis the two side cells are L_(i-1) and L_i.  Whether the device then has them in flight together is the compiler's and the
    // look-up's affair: DESIGN 7p has what was measured.
    const bool diagonal = l.pa != qa && l.pb != qb;  // the route's rule: such a step needs both cells it passes between
    const bool s1 = solid(va + l.sa * l.pa, vb + l.sb * qb), s2 = solid(va + l.sa * qa, vb + l.sb * l.pb), s3 = solid(va + l.sa * l.pa, vb + l.sb * l.pb);
    if ((diagonal & (s1 | s2)) | ((i < l.n) & s3)) return false;
  }
  return true;
}

// Rule 1 over the two arrays.
struct WaySolid {
  const uint8_t* blocked;
  const uint32_t* dist2;  // or null
  uint32_t min_dist2;
  int nb;
  WAY_HD bool operator()(int ia, int ib) const {
    const size_t v = (size_t)ia * (size_t)nb + (size_t)ib;
    return blocked[v] != 0 || (dist2 && dist2[v] < min_dist2);
  }
};

// The defaults for a route and the clearance it read: the route's grid and max_path, a look of 64 cells, no distance kept, 256
// waypoints a path, the clearance's cell_size.  None of it is tuned on real data.
inline int way_default_params(const svo_grid_route_params* r, const svo_grid_clearance_params* c, svo_grid_waypoint_params* p) {
  if (!r || !c || !p) return SVO_ERR_INVALID;
  if (!way_shape_ok(r->na, r->nb) || r->max_path < 1 || r->max_path > WAY_MAX_STRIDE) return SVO_ERR_INVALID;
  if (!(c->cell_size > 0.0 && c->cell_size <= DBL_MAX)) return SVO_ERR_INVALID;
  p->na = r->na; p->nb = r->nb;
  p->path_stride = r->max_path;
  p->max_look = 64;
  p->min_dist2 = 0u;
  p->max_way = 256;
  p->cell_size = c->cell_size;
  return SVO_OK;
}
#endif  // SVO_WAYPOINT_ARGS_H_
