// Ground plan waypoints (include/svo.h, "Ground plan waypoints"): per path of a route the few cells between which a vehicle
// may drive in straight lines, on the context's stream.  One memset and one launch:
//
//   way_kernel : one workgroup per path.  It reads the path's length and status, and all its threads look through the available
//                entries for one outside the grid; a skipped path writes its three words and leaves.  Then the greedy of rule 5: for
//                the current waypoint k thread t takes the candidate j = k + 1 + t (at most max_look <= 255 of them) and walks rule
//                3's line to it by remainders (host/waypoint_args.h), reading blocked (and dist2) as it goes and leaving at the first
//                SOLID cell; the largest clear j comes from one __ballot per wavefront and one LDS word per wavefront,
//                double-buffered so that one barrier a waypoint suffices.
//                No clear j at all is a forced step to k + 1.  Thread 0 writes the waypoint and adds its segment's length, in order.
//
// How the workgroups of one launch agree: only through relaxed device-scope integer atomics whose final value does not
// depend on order (add, max), one of each per path and non-zero count.  No fence, no spinning, no scratch; every loop is bounded by
// max_look <= 255 or by m <= 2^20 as read once, whatever memory holds, and a cell index is range-checked where it is used.
// Checks, the line, CLEAR and the defaults are host/waypoint_args.h's.  A form that staged the window around the waypoint in LDS and
// one of 1,024 threads were measured and dropped.
#include "waypoint_args.h"
#include "kernels.h"

namespace {
using u64 = unsigned long long;
constexpr int WY_T = WAY_THREADS;

struct WayArgs {
  const uint8_t* blocked;
  const uint32_t* dist2;        // or null
  const uint32_t* path;
  const uint32_t* path_len;
  const uint8_t* path_status;   // or null
  uint32_t* way;                // the outputs, null each
  uint32_t* way_index;
  uint32_t* way_len;
  uint8_t* way_status;
  double* length;
  u64* counts;                  // or null
  double cell_size;
  uint32_t n;                   // na * nb, at most 2^24
  uint32_t min_dist2, stride, max_way;
  int na, nb, look;
};
}  // namespace

__global__ __launch_bounds__(WY_T) void way_kernel(WayArgs a) {
  constexpr int T = WY_T;
  __shared__ int sTop[2][T / 64];     // per wavefront the largest clear candidate, or -1; by the waypoint's parity
  constexpr int DEV = __HIP_MEMORY_SCOPE_AGENT;
  const int tid = threadIdx.x;
  const uint32_t p = blockIdx.x;
  const uint32_t* const base = a.path + (size_t)p * a.stride;
  const uint32_t len = a.path_len[p];
  const uint32_t m = len < a.stride ? len : a.stride;
  const unsigned st = a.path_status ? a.path_status[p] : (unsigned)SVO_GRID_ROUTE_OK;
  int why = (st == SVO_GRID_ROUTE_OK || st == SVO_GRID_ROUTE_TRUNCATED) && m >= 1u ? 0 : SVO_GRID_WAY_SKIPPED;
  if (!why) {  // uniform over the workgroup
    int outside = 0;
    for (uint32_t i = (uint32_t)tid; i < m; i += (uint32_t)T) outside |= base[i] >= a.n ? 1 : 0;
    if (__syncthreads_or(outside)) why = SVO_GRID_WAY_BAD_CELL;
  }
  if (why) {
    if (tid == 0) {
      if (a.way_len) a.way_len[p] = 0u;
      if (a.way_status) a.way_status[p] = (uint8_t)why;
      if (a.length) a.length[p] = 0.0;
      if (a.counts) __hip_atomic_fetch_add(&a.counts[1], 1ull, __ATOMIC_RELAXED, DEV);
    }
    return;
  }
  const WaySolid solid{a.blocked, a.dist2, a.min_dist2, a.nb};
  uint32_t k = 0u, w = 1u, n_forced = 0u;  // w, n_forced, max_d2 and s are thread 0's
  u64 max_d2 = 0ull;
  double s = 0.0;
  if (tid == 0) {
    if (a.way) a.way[(size_t)p * a.max_way] = base[0];
    if (a.way_index) a.way_index[(size_t)p * a.max_way] = 0u;
  }
  for (uint32_t it = 0u; k + 1u < m; ++it) {  // k grows by one at least: fewer than m turns
    const uint32_t hi = k + (uint32_t)a.look < m - 1u ? k + (uint32_t)a.look : m - 1u;
    const uint32_t v = base[k];
    const int va = (int)(v / (uint32_t)a.nb), vb = (int)(v - (uint32_t)va * (uint32_t)a.nb);
    const uint32_t j = k + 1u + (uint32_t)tid;
    bool clear = false;
    if (j <= hi && v < a.n) {
      const uint32_t t = base[j];
      if (t < a.n) {
        const int ta = (int)(t / (uint32_t)a.nb), tb = (int)(t - (uint32_t)ta * (uint32_t)a.nb);
        clear = way_clear(va, vb, ta, tb, a.look, solid);
      }
    }
    const u64 lanes = __ballot(clear);
    if ((tid & 63) == 0) sTop[it & 1u][tid >> 6] = lanes ? tid + 63 - __clzll((long long)lanes) : -1;
    __syncthreads();
    int top = -1;
#pragma unroll
    for (int q = 0; q < T / 64; ++q) top = sTop[it & 1u][q] > top ? sTop[it & 1u][q] : top;
    const uint32_t kn = k + 1u + (uint32_t)(top < 0 ? 0 : top);
    if (tid == 0) {
      const uint32_t t = base[kn];
      const long long da = (long long)(t / (uint32_t)a.nb) - va, db = (long long)(t % (uint32_t)a.nb) - vb;
      const u64 d2 = (u64)(da * da + db * db);
      s += sqrt((double)d2);
      max_d2 = d2 > max_d2 ? d2 : max_d2;
      n_forced += top < 0 ? 1u : 0u;
      if (w < a.max_way) {
        if (a.way) a.way[(size_t)p * a.max_way + w] = t;
        if (a.way_index) a.way_index[(size_t)p * a.max_way + w] = kn;
      }
      ++w;
    }
    k = kn;
  }
  if (tid == 0) {
    const bool full = w > a.max_way;
    if (a.way_len) a.way_len[p] = w;
    if (a.way_status) a.way_status[p] = (uint8_t)((len > a.stride ? SVO_GRID_WAY_PATH_TRUNCATED : 0) | (full ? SVO_GRID_WAY_FULL : 0));
    if (a.length) a.length[p] = s * a.cell_size;
    if (a.counts) {
      __hip_atomic_fetch_add(&a.counts[0], 1ull, __ATOMIC_RELAXED, DEV);
      __hip_atomic_fetch_add(&a.counts[2], (u64)m, __ATOMIC_RELAXED, DEV);
      __hip_atomic_fetch_add(&a.counts[3], (u64)w, __ATOMIC_RELAXED, DEV);
      if (n_forced) __hip_atomic_fetch_add(&a.counts[4], (u64)n_forced, __ATOMIC_RELAXED, DEV);
      if (full) __hip_atomic_fetch_add(&a.counts[5], 1ull, __ATOMIC_RELAXED, DEV);
      if (max_d2) __hip_atomic_fetch_max(&a.counts[6], max_d2, __ATOMIC_RELAXED, DEV);
    }
  }
}

// ----------------------------------------------------------------------------- host side
extern "C" int svo_grid_waypoints_default_params(const svo_grid_route_params* route, const svo_grid_clearance_params* clearance,
                                                 svo_grid_waypoint_params* out) {
  return way_default_params(route, clearance, out);
}

extern "C" int svo_grid_waypoints_dev(svo_ctx* ctx, const uint8_t* blocked, const uint32_t* dist2, const uint32_t* path,
                                      const uint32_t* path_len, const uint8_t* path_status, int n_paths,
                                      const svo_grid_waypoint_params* prm, const svo_grid_waypoint_out* out, uint64_t* counts) {
  if (!ctx) return SVO_ERR_INVALID;
  svo_use_device(ctx);
  SVO_ARGS_CHECK(ctx, way_check(blocked, dist2, path, path_len, n_paths, prm, out, counts, true, &err));
  WayArgs a{};
  a.blocked = blocked; a.dist2 = dist2; a.path = path; a.path_len = path_len; a.path_status = path_status;
  a.way = out->way; a.way_index = out->way_index; a.way_len = out->way_len; a.way_status = out->way_status; a.length = out->length;
  a.counts = reinterpret_cast<u64*>(counts);
  a.cell_size = prm->cell_size;
  a.n = (uint32_t)prm->na * (uint32_t)prm->nb; a.min_dist2 = prm->min_dist2; a.stride = (uint32_t)prm->path_stride; a.max_way = (uint32_t)prm->max_way;
  a.na = prm->na; a.nb = prm->nb; a.look = prm->max_look;
  static_assert(WAY_MAX_LOOK < WAY_THREADS, "one candidate per thread");
  const dim3 grid((unsigned)n_paths);
  hipStream_t st = ctx->stream;
  SvoProfScope prof(ctx, SVO_PROF_GRID_WAYPOINTS);
  if (counts) SVO_HIP_CHECK(ctx, hipMemsetAsync(counts, 0, 8 * sizeof(u64), st));
  hipLaunchKernelGGL(way_kernel, grid, dim3(WY_T), 0, st, a);
  SVO_HIP_CHECK(ctx, hipGetLastError());
  return SVO_OK;
}

extern "C" int svo_grid_waypoints(svo_ctx* ctx, const uint8_t* blocked, const uint32_t* dist2, const uint32_t* path, const uint32_t* path_len,
                                  const uint8_t* path_status, int n_paths, const svo_grid_waypoint_params* prm,
                                  const svo_grid_waypoint_out* out, uint64_t* counts) {
  if (!ctx) return SVO_ERR_INVALID;
  svo_use_device(ctx);
  SVO_ARGS_CHECK(ctx, way_check(blocked, dist2, path, path_len, n_paths, prm, out, counts, false, &err));
  const size_t n = (size_t)prm->na * (size_t)prm->nb, np = (size_t)n_paths;
  const size_t b_path = 4 * np * (size_t)prm->path_stride, b_way = 4 * np * (size_t)prm->max_way;
  SvoParts parts;
  const size_t o_counts = parts.add(8 * sizeof(u64)), o_length = parts.add(8 * np), o_way = parts.add(b_way), o_index = parts.add(b_way),
               o_len = parts.add(4 * np), o_status = parts.add(np), o_path = parts.add(b_path), o_plen = parts.add(4 * np), o_pst = parts.add(np),
               o_dist2 = parts.add(4 * n), o_blocked = parts.add(n);
  SvoTemp d;
  SVO_HIP_CHECK(ctx, hipMalloc(&d.p, parts.total()));
  svo_grid_waypoint_out o{};
  o.way = out->way ? d.at<uint32_t>(o_way) : nullptr;  // what the caller did not ask for is not written
  o.way_index = out->way_index ? d.at<uint32_t>(o_index) : nullptr;
  o.way_len = out->way_len ? d.at<uint32_t>(o_len) : nullptr;
  o.way_status = out->way_status ? d.at(o_status) : nullptr;
  o.length = out->length ? d.at<double>(o_length) : nullptr;
  u64 c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  hipStream_t st = ctx->stream;
  hipError_t e = hipMemcpyAsync(d.at(o_blocked), blocked, n, hipMemcpyHostToDevice, st);
  if (e == hipSuccess && dist2) e = hipMemcpyAsync(d.at(o_dist2), dist2, 4 * n, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d.at(o_path), path, b_path, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d.at(o_plen), path_len, 4 * np, hipMemcpyHostToDevice, st);
  if (e == hipSuccess && path_status) e = hipMemcpyAsync(d.at(o_pst), path_status, np, hipMemcpyHostToDevice, st);
  if (e == hipSuccess && out->way) e = hipMemcpyAsync(o.way, out->way, b_way, hipMemcpyHostToDevice, st);  // the untouched entries come back
  if (e == hipSuccess && out->way_index) e = hipMemcpyAsync(o.way_index, out->way_index, b_way, hipMemcpyHostToDevice, st);
  const int rc = svo_host_call(
      ctx, "grid_waypoints", e,
      [&] {
        return svo_grid_waypoints_dev(ctx, d.at(o_blocked), dist2 ? d.at<uint32_t>(o_dist2) : nullptr, d.at<uint32_t>(o_path), d.at<uint32_t>(o_plen),
                                      path_status ? d.at(o_pst) : nullptr, n_paths, prm, &o, counts ? d.at<uint64_t>(o_counts) : nullptr);
      },
      [&] {
        hipError_t e = hipSuccess;
        if (out->way) e = hipMemcpyAsync(out->way, o.way, b_way, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && out->way_index) e = hipMemcpyAsync(out->way_index, o.way_index, b_way, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && out->way_len) e = hipMemcpyAsync(out->way_len, o.way_len, 4 * np, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && out->way_status) e = hipMemcpyAsync(out->way_status, o.way_status, np, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && out->length) e = hipMemcpyAsync(out->length, o.length, 8 * np, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && counts) e = hipMemcpyAsync(c, d.at(o_counts), sizeof(c), hipMemcpyDeviceToHost, st);
        return e;
      });
  if (rc) return rc;
  if (counts) for (int k = 0; k < 8; ++k) counts[k] = c[k];
  return SVO_OK;
}
