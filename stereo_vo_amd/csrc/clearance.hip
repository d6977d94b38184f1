// Ground plan clearance (include/svo.h, "Ground plan clearance"): per cell of a u8 class grid the exact squared
// distance to the nearest source cell, that cell's index, the distance in map units and the inflation, in two launches on the
// context's stream.
//
//   clearance_row_kernel    : one thread per cell, lanes along ib.  It searches its own row outward, g = 0 .. max_dist, the cell at
//                             ib - g before the one at ib + g, and writes the signed offset jb - ib of the first source it meets
//                             into the workspace, or CLEARANCE_NO_OFFSET.
//   clearance_column_kernel : one thread per cell, lanes along ib, so that every step reads the workspace at (ia -+ g) * nb + ib
//                             coalesced.  It goes outward g = 0, 1, .. over the rows, takes each row's candidate (g^2 + offset^2,
//                             its index) under "smaller d2, then smaller index", and stops when g^2 > best, STRICTLY (a candidate
//                             at g^2 == best with offset 0 in an earlier row still wins the tie), or g > max_dist.  Then the cap,
//                             the disc test, the up to four outputs and the counts.
//
// Both searches take CL_STEPS steps at a time: the batch's loads (at indices clamped into the grid, so that none needs a branch) are
// issued before the first of them is tested, and the tests then run in the steps' order, which leaves every result what the
// step-by-step search gives.  Measured against that form in DESIGN §7k: 52 -> 32 us on the 256 x 256 ground plans.
//
// Every cell is written by exactly one thread and the row pass's words are read only by the next launch, so nothing passes between
// workgroups except the counts' relaxed atomicAdds (one per workgroup and non-zero counter): no fence, no waiting.  Offsets are
// size_t (na * nb <= 2^24 keeps them far below 2^32 all the same).  The arithmetic is integer but for rule 4's f64 square root and
// product.  Checks, R2, sizes and the launch geometry are host/clearance_args.h's.
#include "clearance_args.h"
#include "kernels.h"

namespace {
using u64 = unsigned long long;
constexpr int CL_T = CLEARANCE_THREADS;
constexpr int CL_STEPS = 4;  // search steps whose loads are in flight together

struct ClearanceRowArgs {
  const uint8_t* cls;
  int32_t* offsets;  // the workspace
  size_t n;          // na * nb
  int nb, max_dist;
  uint32_t source_mask;
};

struct ClearanceColumnArgs {
  const int32_t* offsets;
  size_t n;
  int na, nb, max_dist;
  uint32_t r2;  // rule 5's R2, <= max_dist^2
  double cell_size;
  svo_grid_clearance_out o;
  u64* counts;  // 4 (zeroed on the stream before the launch), or null
};

__device__ __forceinline__ bool cl_source(unsigned c, uint32_t mask) { return c < 32u && ((mask >> c) & 1u) != 0u; }
}  // namespace

__global__ __launch_bounds__(CL_T) void clearance_row_kernel(ClearanceRowArgs a) {
  const size_t i = (size_t)blockIdx.x * CL_T + (size_t)threadIdx.x;
  if (i >= a.n) return;
  const int nb = a.nb;
  const int ia = (int)(i / (size_t)nb), ib = (int)(i - (size_t)ia * (size_t)nb);
  const uint8_t* __restrict__ row = a.cls + (size_t)ia * (size_t)nb;
  // beyond the row's nearer end only one side is left, beyond the farther end nothing
  const int reach = min(a.max_dist, max(ib, nb - 1 - ib));
  int32_t off = CLEARANCE_NO_OFFSET;
  // CL_STEPS steps at a time: their loads, at indices clamped into the row, are issued before the first test, so that a wavefront
  // waits for memory once per batch; the tests then run in the steps' order and ignore what a clamp fetched.
  for (int g0 = 0; g0 <= reach && off == CLEARANCE_NO_OFFSET; g0 += CL_STEPS) {
    unsigned left[CL_STEPS], right[CL_STEPS];
#pragma unroll
    for (int k = 0; k < CL_STEPS; ++k) {
      left[k] = row[max(ib - g0 - k, 0)];
      right[k] = row[min(ib + g0 + k, nb - 1)];
    }
#pragma unroll
    for (int k = 0; k < CL_STEPS; ++k) {
      const int g = g0 + k;
      const bool l = ib - g >= 0 && cl_source(left[k], a.source_mask), r = ib + g < nb && cl_source(right[k], a.source_mask);
      const bool open = off == CLEARANCE_NO_OFFSET && g <= reach;
      off = open && l ? -g : (open && r ? g : off);
    }
  }
  a.offsets[i] = off;
}

__global__ __launch_bounds__(CL_T) void clearance_column_kernel(ClearanceColumnArgs a) {
  __shared__ unsigned sC[4][CL_T / 64];
  const int tid = threadIdx.x;
  const size_t i = (size_t)blockIdx.x * CL_T + (size_t)tid;
  unsigned n_src = 0, n_reached = 0, n_unreached = 0, n_blocked = 0;
  if (i < a.n) {
    const int nb = a.nb, na = a.na;
    const int ia = (int)(i / (size_t)nb), ib = (int)(i - (size_t)ia * (size_t)nb);
    const int32_t* __restrict__ col = a.offsets + ib;
    const int reach = min(a.max_dist, max(ia, na - 1 - ia));
    uint32_t best = CLEARANCE_NONE, at = CLEARANCE_NONE;
    auto take = [&](int32_t word, int ja, uint32_t g2, bool on) {
      const bool some = word != CLEARANCE_NO_OFFSET;
      const int o = some ? word : 0;  // |o| <= 8191
      const uint32_t d2 = g2 + (uint32_t)(o * o), j = (uint32_t)(ja * nb + ib + o);  // j < 2^24 where `on`
      const bool wins = on && some && (d2 < best || (d2 == best && j < at));
      best = wins ? d2 : best;
      at = wins ? j : at;
    };
    // CL_STEPS rows either way at a time, loaded (at rows clamped into the grid) before the first is looked at.  Within a batch a
    // step past the stop g * g > best is skipped, which is the stop: best only falls and g * g only grows.
    for (int g0 = 0; g0 <= reach && (uint32_t)(g0 * g0) <= best; g0 += CL_STEPS) {
      int32_t up[CL_STEPS], down[CL_STEPS];
#pragma unroll
      for (int k = 0; k < CL_STEPS; ++k) {
        up[k] = col[(size_t)max(ia - g0 - k, 0) * (size_t)nb];
        down[k] = col[(size_t)min(ia + g0 + k, na - 1) * (size_t)nb];
      }
#pragma unroll
      for (int k = 0; k < CL_STEPS; ++k) {
        const int g = g0 + k;
        const uint32_t g2 = (uint32_t)(g * g);
        const bool on = g <= reach && g2 <= best;
        take(up[k], ia - g, g2, on && ia - g >= 0);
        take(down[k], ia + g, g2, on && g > 0 && ia + g < na);
      }
    }
    if (best != CLEARANCE_NONE && best > (uint32_t)(a.max_dist * a.max_dist)) { best = CLEARANCE_NONE; at = CLEARANCE_NONE; }
    const bool none = best == CLEARANCE_NONE, src = best == 0u;
    const uint8_t blocked = src ? 2 : (!none && best <= a.r2 ? 1 : 0);
    a.o.dist2[i] = best;
    if (a.o.nearest) a.o.nearest[i] = at;
    if (a.o.clearance) a.o.clearance[i] = none ? __builtin_inff() : (float)(sqrt((double)best) * a.cell_size);
    if (a.o.blocked) a.o.blocked[i] = blocked;
    n_src = src ? 1u : 0u;
    n_reached = !src && !none ? 1u : 0u;
    n_unreached = none ? 1u : 0u;
    n_blocked = blocked == 1 ? 1u : 0u;
  }
  if (!a.counts) return;  // uniform over the launch
  for (int o = 32; o > 0; o >>= 1) {
    n_src += __shfl_xor(n_src, o);
    n_reached += __shfl_xor(n_reached, o);
    n_unreached += __shfl_xor(n_unreached, o);
    n_blocked += __shfl_xor(n_blocked, o);
  }
  if ((tid & 63) == 0) {
    sC[0][tid >> 6] = n_src; sC[1][tid >> 6] = n_reached; sC[2][tid >> 6] = n_unreached; sC[3][tid >> 6] = n_blocked;
  }
  __syncthreads();
  if (tid < 4) {
    unsigned t = 0;
    for (int w = 0; w < CL_T / 64; ++w) t += sC[tid][w];
    if (t) __hip_atomic_fetch_add(&a.counts[tid], (u64)t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ----------------------------------------------------------------------------- host side
extern "C" int svo_grid_clearance_default_params(const svo_voxel_grid_params* grid, float voxel_size, svo_grid_clearance_params* out) {
  return clearance_default_params(grid, voxel_size, out);
}

extern "C" size_t svo_grid_clearance_workspace_bytes(int na, int nb) { return clearance_workspace_bytes(na, nb); }

extern "C" int svo_grid_clearance_dev(svo_ctx* ctx, const uint8_t* cls, const svo_grid_clearance_params* prm, void* workspace,
                                      const svo_grid_clearance_out* out, uint64_t* counts) {
  if (!ctx) return SVO_ERR_INVALID;
  svo_use_device(ctx);
  SVO_ARGS_CHECK(ctx, clearance_check(cls, prm, workspace, out, counts, &err));
  ClearanceRowArgs a{};
  a.cls = cls; a.offsets = static_cast<int32_t*>(workspace);
  a.n = (size_t)prm->na * (size_t)prm->nb;
  a.nb = prm->nb; a.max_dist = prm->max_dist; a.source_mask = prm->source_mask;
  ClearanceColumnArgs b{};
  b.offsets = a.offsets; b.n = a.n;
  b.na = prm->na; b.nb = prm->nb; b.max_dist = prm->max_dist;
  b.r2 = clearance_r2(prm);
  b.cell_size = prm->cell_size;
  b.o = *out;
  b.counts = reinterpret_cast<u64*>(counts);
  const dim3 groups((unsigned)clearance_groups(a.n));
  SvoProfScope prof(ctx, SVO_PROF_GRID_CLEARANCE);
  if (counts) SVO_HIP_CHECK(ctx, hipMemsetAsync(counts, 0, 4 * sizeof(u64), ctx->stream));
  hipLaunchKernelGGL(clearance_row_kernel, groups, dim3(CL_T), 0, ctx->stream, a);
  SVO_HIP_CHECK(ctx, hipGetLastError());
  hipLaunchKernelGGL(clearance_column_kernel, groups, dim3(CL_T), 0, ctx->stream, b);
  SVO_HIP_CHECK(ctx, hipGetLastError());
  return SVO_OK;
}

extern "C" int svo_grid_clearance(svo_ctx* ctx, const uint8_t* cls, const svo_grid_clearance_params* prm, const svo_grid_clearance_out* out,
                                  uint64_t* counts) {
  if (!ctx) return SVO_ERR_INVALID;
  svo_use_device(ctx);
  SVO_REQUIRE(ctx, cls, "grid_clearance: null cls");
  SVO_ARGS_CHECK(ctx, clearance_params_check(prm, &err));
  SVO_ARGS_CHECK(ctx, clearance_out_check(out, false, &err));
  const size_t n = (size_t)prm->na * (size_t)prm->nb;
  SvoParts parts;
  const size_t o_counts = parts.add(4 * sizeof(u64)), o_ws = parts.add(clearance_workspace_bytes(prm->na, prm->nb)), o_dist2 = parts.add(4 * n),
               o_nearest = parts.add(4 * n), o_clearance = parts.add(4 * n), o_blocked = parts.add(n), o_cls = parts.add(n);
  SvoTemp d;
  SVO_HIP_CHECK(ctx, hipMalloc(&d.p, parts.total()));
  svo_grid_clearance_out o{};
  o.dist2 = d.at<uint32_t>(o_dist2);
  o.nearest = out->nearest ? d.at<uint32_t>(o_nearest) : nullptr;  // what the caller did not ask for is not written
  o.clearance = out->clearance ? d.at<float>(o_clearance) : nullptr;
  o.blocked = out->blocked ? d.at(o_blocked) : nullptr;
  u64 c[4] = {0, 0, 0, 0};
  hipStream_t st = ctx->stream;
  const int rc = svo_host_call(
      ctx, "grid_clearance", hipMemcpyAsync(d.at(o_cls), cls, n, hipMemcpyHostToDevice, st),
      [&] { return svo_grid_clearance_dev(ctx, d.at(o_cls), prm, d.at(o_ws), &o, d.at<uint64_t>(o_counts)); },
      [&] {
        hipError_t e = hipMemcpyAsync(out->dist2, o.dist2, 4 * n, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && out->nearest) e = hipMemcpyAsync(out->nearest, o.nearest, 4 * n, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && out->clearance) e = hipMemcpyAsync(out->clearance, o.clearance, 4 * n, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && out->blocked) e = hipMemcpyAsync(out->blocked, o.blocked, n, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(c, d.at(o_counts), sizeof(c), hipMemcpyDeviceToHost, st);
        return e;
      });
  if (rc) return rc;
  if (counts) for (int k = 0; k < 4; ++k) counts[k] = c[k];
  return SVO_OK;
}
