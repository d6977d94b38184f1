// Ground plan surface (include/svo.h, "Ground plan surface"): from the grid's cls and top, per cell, the largest height
// step to an edge neighbour, the relief and the support under a disc-shaped footprint, and a refined class grid, in one launch on
// the context's stream.
//
//   surface_kernel : a workgroup of 256 takes tiles of SURFACE_TILE_A x SURFACE_TILE_B cells, one cell per thread, lanes along ib:
//                    one tile where the grid has at most SURFACE_MAX_GROUPS of them, otherwise tiles g, g + groups, ... in turn.
//                    It stages the tile and a halo of max(rw, 1) cells into LDS as one float per cell: the top of a GROUND cell,
//                    and a NaN, "nothing there", for a cell outside the grid (an integer test on the indices) or not GROUND.  A
//                    GROUND top is finite, so the word holds the flag and the height at once.  Then every thread takes its cell's
//                    step from the four staged neighbours (f64 subtractions) and walks the disc row by row, the half widths from
//                    the table in the launch's arguments, for hi, lo and the support; compares select, they never add, so the
//                    order of the walk is not in the result.  Rule 6, the up to four stores, and the six tallies by __ballot /
//                    __popcll per wavefront and tile, kept in registers over the workgroup's tiles; at the end one LDS add per
//                    wavefront and tally and one global add per workgroup and non-zero tally.
//
// Every cell is written by exactly one thread and nothing is read that the launch writes: no atomics but the counts', no fence, no
// waiting.  Every loop is bounded by rw <= 15, by the window or by the workgroup's share of the tiles (at most ceil(tiles / groups)
// turns, at most 17 for 2^24 cells); byte offsets are size_t.  Checks, the footprint, the tile and the launch geometry are
// host/surface_args.h's.
#include "surface_args.h"
#include "kernels.h"

namespace {
using u64 = unsigned long long;
constexpr int SF_T = SURFACE_THREADS, SF_TA = SURFACE_TILE_A, SF_TB = SURFACE_TILE_B, SF_S = SURFACE_LDS_STRIDE;

struct SurfaceArgs {
  const uint8_t* cls;
  const float* top;
  svo_grid_surface_out o;
  u64* counts;  // 6 (zeroed on the stream before the launch), or null
  int na, nb, rw, halo;
  unsigned tiles, tiles_b;      // the tiles of the grid, and those along ib
  uint32_t ground_mask, cells, min_support_256;
  double max_step, max_relief;
  uint8_t w[SURFACE_ROWS + 1];  // w[rw + da], da = -rw .. rw
};

__device__ __forceinline__ bool sf_in_mask(unsigned c, uint32_t mask) { return c < 32u && ((mask >> (c & 31u)) & 1u) != 0u; }
__device__ __forceinline__ bool sf_finite(float t) { return __builtin_fabsf(t) <= FLT_MAX; }  // false for a NaN
}  // namespace

__global__ __launch_bounds__(SF_T) void surface_kernel(SurfaceArgs a) {
  __shared__ float sTop[SURFACE_LDS_ROWS * SF_S];
  __shared__ unsigned sN[6];
  const int tid = threadIdx.x;
  const int h = a.halo, wa = SF_TA + 2 * h, wb = SF_TB + 2 * h;  // the window: wa <= SURFACE_LDS_ROWS rows of wb <= SF_S cells
  const int la = tid / SF_TB, lb = tid - la * SF_TB;
  if (tid < 6) sN[tid] = 0u;
  unsigned n_ground = 0, n_step = 0, n_rough = 0, n_unsup = 0, n_nonfinite = 0, n_kept = 0;  // the same in every lane of a wavefront
  for (unsigned tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {  // at most ceil(tiles / groups) turns, the same for every thread
    const int a0 = (int)(tile / a.tiles_b) * SF_TA, b0 = (int)(tile % a.tiles_b) * SF_TB;
    for (int idx = tid; idx < wa * wb; idx += SF_T) {
      const int ra = idx / wb, rb = idx - ra * wb;
      const int ga = a0 - h + ra, gb = b0 - h + rb;
      float v = __builtin_nanf("");
      if (ga >= 0 && ga < a.na && gb >= 0 && gb < a.nb) {
        const size_t i = (size_t)ga * (size_t)a.nb + (size_t)gb;
        const unsigned c = a.cls[i];
        const float t = a.top[i];
        if (sf_in_mask(c, a.ground_mask) && sf_finite(t)) v = t;
      }
      sTop[ra * SF_S + rb] = v;
    }
    __syncthreads();
    const int ia = a0 + la, ib = b0 + lb;
    const bool in = ia < a.na && ib < a.nb;
    bool ground = false, is_step = false, is_rough = false, is_unsup = false, nonfinite = false, kept = false;
    if (in) {
      const size_t i = (size_t)ia * (size_t)a.nb + (size_t)ib;
      const unsigned c = a.cls[i];
      const float* const ctr = sTop + (la + h) * SF_S + (lb + h);
      const float t = *ctr;
      ground = t == t;
      nonfinite = !ground && sf_in_mask(c, a.ground_mask);
      // rule 3: the four edge neighbours; a NaN fails the test
      double dstep = 0.0;
      if (ground) {
        const float nbr[4] = {ctr[-SF_S], ctr[-1], ctr[1], ctr[SF_S]};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const double d = __builtin_fabs((double)t - (double)nbr[k]);
          dstep = nbr[k] == nbr[k] && d > dstep ? d : dstep;
        }
      }
      // rules 4 and 5: the disc, row by row; every comparison with a NaN is false
      float hi = -__builtin_inff(), lo = __builtin_inff();
      unsigned support = 0u;
      for (int da = -a.rw; da <= a.rw; ++da) {  // rw <= 15
        const int w = a.w[a.rw + da];
        const float* const row = ctr + da * SF_S;
        for (int db = -w; db <= w; ++db) {      // w <= rw
          const float v = row[db];
          support += v == v ? 1u : 0u;
          hi = v > hi ? v : hi;
          lo = v < lo ? v : lo;
        }
      }
      const double drelief = hi > lo ? (double)hi - (double)lo : 0.0;
      // rule 6
      unsigned out = c;
      if (ground) {
        is_step = dstep > a.max_step;
        is_rough = !is_step && drelief > a.max_relief;
        is_unsup = !is_step && !is_rough && surface_unsupported(support, a.min_support_256, a.cells);
        kept = !is_step && !is_rough && !is_unsup;
        out = is_step ? SVO_GRID_SURFACE_STEP : is_rough ? SVO_GRID_SURFACE_ROUGH : is_unsup ? SVO_GRID_SURFACE_UNSUPPORTED : c;
      } else if (nonfinite) {
        out = SVO_GRID_SURFACE_UNSUPPORTED;
      }
      a.o.cls_out[i] = (uint8_t)out;
      if (a.o.step) a.o.step[i] = ground ? (float)dstep : -1.0f;
      if (a.o.relief) a.o.relief[i] = ground ? (float)drelief : -1.0f;
      if (a.o.support) a.o.support[i] = (uint16_t)support;
    }
    if (a.counts) {  // uniform over the launch
      n_ground += (unsigned)__popcll(__ballot(ground));
      n_step += (unsigned)__popcll(__ballot(is_step));
      n_rough += (unsigned)__popcll(__ballot(is_rough));
      n_unsup += (unsigned)__popcll(__ballot(is_unsup));
      n_nonfinite += (unsigned)__popcll(__ballot(nonfinite));
      n_kept += (unsigned)__popcll(__ballot(kept));
    }
    __syncthreads();  // the window is read to its end before the next tile is staged over it
  }
  if (!a.counts) return;  // uniform over the launch
  if ((tid & 63) == 0) {
    constexpr int WG = __HIP_MEMORY_SCOPE_WORKGROUP;
    __hip_atomic_fetch_add(&sN[0], n_ground, __ATOMIC_RELAXED, WG);
    __hip_atomic_fetch_add(&sN[1], n_step, __ATOMIC_RELAXED, WG);
    __hip_atomic_fetch_add(&sN[2], n_rough, __ATOMIC_RELAXED, WG);
    __hip_atomic_fetch_add(&sN[3], n_unsup, __ATOMIC_RELAXED, WG);
    __hip_atomic_fetch_add(&sN[4], n_nonfinite, __ATOMIC_RELAXED, WG);
    __hip_atomic_fetch_add(&sN[5], n_kept, __ATOMIC_RELAXED, WG);
  }
  __syncthreads();
  if (tid < 6) {
    const unsigned t = sN[tid];
    if (t) __hip_atomic_fetch_add(&a.counts[tid], (u64)t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ----------------------------------------------------------------------------- host side
extern "C" int svo_grid_surface_default_params(const svo_voxel_grid_params* grid, float voxel_size, svo_grid_surface_params* out) {
  return surface_default_params(grid, voxel_size, out);
}

extern "C" uint32_t svo_grid_surface_footprint_cells(uint32_t r2) { return surface_footprint_cells(r2); }

extern "C" int svo_grid_surface_dev(svo_ctx* ctx, const uint8_t* cls, const float* top, const svo_grid_surface_params* prm,
                                    const svo_grid_surface_out* out, uint64_t* counts) {
  if (!ctx) return SVO_ERR_INVALID;
  svo_use_device(ctx);
  SVO_ARGS_CHECK(ctx, surface_check(cls, top, prm, out, counts, true, &err));
  const SurfaceFootprint f = surface_footprint(surface_r2(prm));
  SurfaceArgs a{};
  a.cls = cls; a.top = top; a.o = *out;
  a.counts = reinterpret_cast<u64*>(counts);
  a.na = prm->na; a.nb = prm->nb; a.rw = f.rw; a.halo = surface_halo(f.rw);
  a.ground_mask = prm->ground_mask; a.cells = f.cells; a.min_support_256 = (uint32_t)prm->min_support_256;
  a.max_step = prm->max_step; a.max_relief = prm->max_relief;
  static_assert(sizeof(a.w) == sizeof(f.w), "the half-width table");
  memcpy(a.w, f.w, sizeof(a.w));
  a.tiles_b = surface_tiles_b(prm->nb); a.tiles = surface_tiles_a(prm->na) * a.tiles_b;
  const dim3 groups(surface_groups(a.tiles));
  SvoProfScope prof(ctx, SVO_PROF_GRID_SURFACE);
  if (counts) SVO_HIP_CHECK(ctx, hipMemsetAsync(counts, 0, 6 * sizeof(u64), ctx->stream));
  hipLaunchKernelGGL(surface_kernel, groups, dim3(SF_T), 0, ctx->stream, a);
  SVO_HIP_CHECK(ctx, hipGetLastError());
  return SVO_OK;
}

extern "C" int svo_grid_surface(svo_ctx* ctx, const uint8_t* cls, const float* top, const svo_grid_surface_params* prm,
                                const svo_grid_surface_out* out, uint64_t* counts) {
  if (!ctx) return SVO_ERR_INVALID;
  svo_use_device(ctx);
  SVO_ARGS_CHECK(ctx, surface_check(cls, top, prm, out, counts, false, &err));
  const size_t n = (size_t)prm->na * (size_t)prm->nb;
  SvoParts parts;
  const size_t o_counts = parts.add(6 * sizeof(u64)), o_top = parts.add(4 * n), o_step = parts.add(4 * n), o_relief = parts.add(4 * n),
               o_support = parts.add(2 * n), o_cls = parts.add(n), o_cls_out = parts.add(n);
  SvoTemp d;
  SVO_HIP_CHECK(ctx, hipMalloc(&d.p, parts.total()));
  svo_grid_surface_out o{};
  o.cls_out = d.at(o_cls_out);
  o.step = out->step ? d.at<float>(o_step) : nullptr;  // what the caller did not ask for is not written
  o.relief = out->relief ? d.at<float>(o_relief) : nullptr;
  o.support = out->support ? d.at<uint16_t>(o_support) : nullptr;
  u64 c[6] = {0, 0, 0, 0, 0, 0};
  hipStream_t st = ctx->stream;
  hipError_t e = hipMemcpyAsync(d.at(o_cls), cls, n, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d.at(o_top), top, 4 * n, hipMemcpyHostToDevice, st);
  const int rc = svo_host_call(
      ctx, "grid_surface", e, [&] { return svo_grid_surface_dev(ctx, d.at(o_cls), d.at<float>(o_top), prm, &o, d.at<uint64_t>(o_counts)); },
      [&] {
        hipError_t e = hipMemcpyAsync(out->cls_out, o.cls_out, n, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && out->step) e = hipMemcpyAsync(out->step, o.step, 4 * n, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && out->relief) e = hipMemcpyAsync(out->relief, o.relief, 4 * n, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && out->support) e = hipMemcpyAsync(out->support, o.support, 2 * n, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(c, d.at(o_counts), sizeof(c), hipMemcpyDeviceToHost, st);
        return e;
      });
  if (rc) return rc;
  if (counts) for (int k = 0; k < 6; ++k) counts[k] = c[k];
  return SVO_OK;
}
