// The ground plan surface's host logic that needs no GPU (include/svo.h, "Ground plan surface"): the parameter and
// pointer checks with their message texts and their order, the footprint (r2, the per-row half widths, D), the support comparison,
// the tile, the launch geometry and the defaults.  A refusal is SVO_ERR_INVALID with *err set to the message; csrc/surface.hip
// stores it in the context and keeps no second copy of anything here.  tests/sanitize/grid_surface_args_test.cpp walks every
// refusal at its boundary and the footprint table on a CPU.
#ifndef SVO_SURFACE_ARGS_H_
#define SVO_SURFACE_ARGS_H_
#include <float.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "svo.h"

#if defined(__HIPCC__)
#define SURFACE_HD __host__ __device__
#else
#define SURFACE_HD
#endif

#define SURFACE_REFUSE(cond, msg) do { if (!(cond)) { *err = (msg); return SVO_ERR_INVALID; } } while (0)

// The tile of cells one workgroup takes, one cell per thread.  8 x 32 was measured against 16 x 16 and 4 x 64; a
// developer build may set another shape of 256 cells (-DSVO_EXP_SURFACE_TILE_A=.. -DSVO_EXP_SURFACE_TILE_B=..) to measure it again.
#if defined(SVO_EXP_SURFACE_TILE_A) && defined(SVO_EXP_SURFACE_TILE_B)
constexpr int SURFACE_TILE_A = SVO_EXP_SURFACE_TILE_A, SURFACE_TILE_B = SVO_EXP_SURFACE_TILE_B;
#else
constexpr int SURFACE_TILE_A = 8, SURFACE_TILE_B = 32;
#endif
constexpr int SURFACE_THREADS = 256;
static_assert(SURFACE_TILE_A * SURFACE_TILE_B == SURFACE_THREADS, "one cell per thread");
constexpr int SURFACE_MAX_SIDE = 8192;
constexpr long long SURFACE_MAX_CELLS = 1ll << 24;
constexpr int SURFACE_MAX_RW = 15;                   // the footprint reaches at most 15 cells each way:
constexpr double SURFACE_RC2_LIMIT = 226.0;          // rc * rc >= 226 is refused, so r2 <= 225
constexpr uint32_t SURFACE_MAX_R2 = 225u;
constexpr int SURFACE_ROWS = 2 * SURFACE_MAX_RW + 1; // the half-width table's entries
constexpr int SURFACE_MAX_SUPPORT_256 = 256;

inline int surface_params_check(const svo_grid_surface_params* p, const char** err) {
  SURFACE_REFUSE(p->na >= 1 && p->na <= SURFACE_MAX_SIDE, "grid_surface: na outside 1..8192");
  SURFACE_REFUSE(p->nb >= 1 && p->nb <= SURFACE_MAX_SIDE, "grid_surface: nb outside 1..8192");
  SURFACE_REFUSE((long long)p->na * p->nb <= SURFACE_MAX_CELLS, "grid_surface: na * nb beyond 2^24");
  SURFACE_REFUSE(p->ground_mask != 0u, "grid_surface: ground_mask is 0");
  SURFACE_REFUSE(p->cell_size > 0.0 && p->cell_size <= DBL_MAX, "grid_surface: cell_size must be finite and > 0");  // a NaN fails the first test
  SURFACE_REFUSE(p->max_step >= 0.0, "grid_surface: max_step must be >= 0 and not NaN");
  SURFACE_REFUSE(p->footprint_radius >= 0.0 && p->footprint_radius <= DBL_MAX, "grid_surface: footprint_radius must be finite and >= 0");
  {
    const double rc = p->footprint_radius / p->cell_size;  // finite or +inf, never NaN after the two tests above
    SURFACE_REFUSE(rc * rc < SURFACE_RC2_LIMIT, "grid_surface: footprint_radius beyond 15 cells (rc * rc >= 226)");
  }
  SURFACE_REFUSE(p->max_relief >= 0.0, "grid_surface: max_relief must be >= 0 and not NaN");
  SURFACE_REFUSE(p->min_support_256 >= 0 && p->min_support_256 <= SURFACE_MAX_SUPPORT_256, "grid_surface: min_support_256 outside 0..256");
  return SVO_OK;
}

// The order of the refusals: the nulls (cls, top, params, out, cls_out), cls_out == cls, every range in the order of the fields
// (the footprint's reach right after footprint_radius), then the 4-byte alignments (top, step, relief), support's 2 bytes and the
// counts' 8.  device: the _dev entry, whose pointers the kernel relies on; the synchronous entry takes host pointers of any alignment.
inline int surface_check(const void* cls, const void* top, const svo_grid_surface_params* p, const svo_grid_surface_out* o, const void* counts,
                         bool device, const char** err) {
  SURFACE_REFUSE(cls, "grid_surface: null cls");
  SURFACE_REFUSE(top, "grid_surface: null top");
  SURFACE_REFUSE(p, "grid_surface: null params");
  SURFACE_REFUSE(o, "grid_surface: null out");
  SURFACE_REFUSE(o->cls_out, "grid_surface: null cls_out");
  SURFACE_REFUSE((const void*)o->cls_out != cls, "grid_surface: cls_out must not be cls");
  if (const int rc = surface_params_check(p, err)) return rc;
  if (!device) return SVO_OK;
  SURFACE_REFUSE(((uintptr_t)top & 3u) == 0, "grid_surface: top must be 4-byte aligned");
  SURFACE_REFUSE(((uintptr_t)o->step & 3u) == 0, "grid_surface: step must be 4-byte aligned");
  SURFACE_REFUSE(((uintptr_t)o->relief & 3u) == 0, "grid_surface: relief must be 4-byte aligned");
  SURFACE_REFUSE(((uintptr_t)o->support & 1u) == 0, "grid_surface: support must be 2-byte aligned");
  SURFACE_REFUSE(((uintptr_t)counts & 7u) == 0, "grid_surface: counts must be 8-byte aligned");
  return SVO_OK;
}

// ----------------------------------------------------------------------------- the footprint
// Rule 2's r2 = (u64)floor(rc * rc), rc = footprint_radius / cell_size: two stated f64 operations and a floor.  p has passed
// surface_params_check, so rc * rc < 226 and nothing here is a NaN.
inline uint32_t surface_r2(const svo_grid_surface_params* p) {
  const double rc = p->footprint_radius / p->cell_size;
  return (uint32_t)floor(rc * rc);
}

// floor(sqrt(v)) for v <= 225, in integers.
SURFACE_HD inline int surface_isqrt(uint32_t v) {
  int s = 0;
  while (s < SURFACE_MAX_RW && (uint32_t)((s + 1) * (s + 1)) <= v) ++s;
  return s;
}

// rw = isqrt(r2); w[rw + da] = isqrt(r2 - da * da) for da = -rw .. rw, the half width of the disc's row da; cells = D(r2), the
// number of offsets (da, db) with da^2 + db^2 <= r2.  Entries beyond 2 rw are 0 and are not read.
struct SurfaceFootprint {
  uint32_t r2, cells;
  int rw;
  uint8_t w[SURFACE_ROWS + 1];
};

inline SurfaceFootprint surface_footprint(uint32_t r2) {
  SurfaceFootprint f{};
  f.r2 = r2 > SURFACE_MAX_R2 ? SURFACE_MAX_R2 : r2;
  f.rw = surface_isqrt(f.r2);
  for (int da = -f.rw; da <= f.rw; ++da) {
    const int w = surface_isqrt(f.r2 - (uint32_t)(da * da));
    f.w[f.rw + da] = (uint8_t)w;
    f.cells += 2u * (uint32_t)w + 1u;
  }
  return f;
}

// D(r2); 0 for an r2 no accepted call has (> 225).
inline uint32_t surface_footprint_cells(uint32_t r2) { return r2 > SURFACE_MAX_R2 ? 0u : surface_footprint(r2).cells; }

// Rule 6c, in u32: support <= D <= 709 and min_support_256 <= 256, so neither product passes 2^18.
SURFACE_HD inline bool surface_unsupported(uint32_t support, uint32_t min_support_256, uint32_t cells) {
  return support * 256u < min_support_256 * cells;
}

// ----------------------------------------------------------------------------- the tile and the launch geometry
// The staged window: the tile and a halo of max(rw, 1) cells each way (rule 3 looks one cell out even where the footprint is the
// cell alone), rows SURFACE_LDS_STRIDE floats apart.
SURFACE_HD inline int surface_halo(int rw) { return rw < 1 ? 1 : rw; }
// A 16-wide tile puts two rows into each 32-lane half of a wavefront: a stride of 48 floats (16 mod 32) keeps them on different
// banks.  Wider tiles put 32 consecutive floats into a half whatever the stride.
constexpr int SURFACE_LDS_STRIDE = SURFACE_TILE_B == 16 ? 48 : SURFACE_TILE_B + 2 * SURFACE_MAX_RW;
constexpr int SURFACE_LDS_ROWS = SURFACE_TILE_A + 2 * SURFACE_MAX_RW;
constexpr size_t SURFACE_LDS_BYTES = sizeof(float) * (size_t)SURFACE_LDS_ROWS * (size_t)SURFACE_LDS_STRIDE;
static_assert(SURFACE_TILE_B + 2 * SURFACE_MAX_RW <= SURFACE_LDS_STRIDE, "a staged row fits its stride");
inline unsigned surface_tiles_a(int na) { return (unsigned)((na + SURFACE_TILE_A - 1) / SURFACE_TILE_A); }
inline unsigned surface_tiles_b(int nb) { return (unsigned)((nb + SURFACE_TILE_B - 1) / SURFACE_TILE_B); }
// The launch: one workgroup per tile up to SURFACE_MAX_GROUPS, beyond that every workgroup takes tiles g, g + groups, ... in turn.
// The cap is there for the counts: every workgroup ends with up to six adds on one cache line, and with one workgroup per tile
// those adds, not the cells, set the time of a large grid.  4,096 was measured against none, 1,024 and 2,048; a
// developer build may set another (-DSVO_EXP_SURFACE_MAX_GROUPS=..).
#if defined(SVO_EXP_SURFACE_MAX_GROUPS)
constexpr unsigned SURFACE_MAX_GROUPS = SVO_EXP_SURFACE_MAX_GROUPS;
#else
constexpr unsigned SURFACE_MAX_GROUPS = 4096;
#endif
inline unsigned surface_groups(unsigned tiles) { return tiles < SURFACE_MAX_GROUPS ? tiles : SURFACE_MAX_GROUPS; }

// The defaults for a grid of svo_voxel_map_grid* (NOT tuned on real data): its shape, its cell edge in map units, LEVEL cells as
// the ground, a step of obstacle_step, a footprint of 1.5 cells (r2 = 2: the cell and its eight neighbours), a relief of twice
// obstacle_step, no support rule.
inline int surface_default_params(const svo_voxel_grid_params* g, float voxel_size, svo_grid_surface_params* p) {
  if (!g || !p || !(voxel_size > 0.0f && voxel_size <= FLT_MAX)) return SVO_ERR_INVALID;
  if (g->cell_voxels < 1 || g->cell_voxels > 1024 || g->na < 1 || g->na > SURFACE_MAX_SIDE || g->nb < 1 || g->nb > SURFACE_MAX_SIDE ||
      (long long)g->na * g->nb > SURFACE_MAX_CELLS || !(g->obstacle_step >= 0.0))
    return SVO_ERR_INVALID;
  p->na = g->na; p->nb = g->nb;
  p->ground_mask = 1u << SVO_VOXEL_GRID_LEVEL;
  p->cell_size = (double)g->cell_voxels * (double)voxel_size;
  p->max_step = g->obstacle_step;
  p->footprint_radius = 1.5 * p->cell_size;
  p->max_relief = 2.0 * g->obstacle_step;
  p->min_support_256 = 0;
  return SVO_OK;
}
#endif  // SVO_SURFACE_ARGS_H_
