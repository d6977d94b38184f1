// Voxel map route (include/svo.h, "Voxel map route"): the cost-to-go field to goal cells through the free space of the
// occupancy entry's bit volume, the first move per cell and the paths from start cells, on the map's stream.  csrc/route.hip's five
// kernels lifted to 26 neighbours.  A Bellman-Ford fixed point with positive integer weights is unique whatever the order of
// relaxation, so the tiled form below gives Dijkstra's field bit for bit once it has converged.
//
//   voxel_route_goals_kernel   : one thread per goal entry (after the memsets that set cost to NONE and zero the workspace's header
//                                and activity words).  A used goal gets cost 0 and marks its tile and the 26 around it in activity
//                                array 0.
//   voxel_route_round_kernel   : enqueued max_rounds times, one workgroup per TX x TY x TZ tile, axis 0 the contiguous one.  A tile
//                                whose word in this round's activity array is 0 exits.  An active one clears the word and stages the
//                                tile with a one-cell halo into LDS: two copies of cost, the unit 16 + pen, and the closed flags,
//                                taken from the bit words (closed is never expanded to bytes in memory).  Each cell's 26-bit
//                                allowed mask is built once.  Then sweeps: every cell takes the minimum over its allowed moves,
//                                read from one copy of the tile and written to the other, one __syncthreads_or, the copies
//                                swapped, until a sweep changes nothing or VOXEL_ROUTE_MAX_SWEEPS are done.  It then writes the
//                                lowered cells back, marks in the OTHER array exactly the neighbour tiles (up to 26) whose halo
//                                holds a fallen border cell, and itself if the sweep bound cut it short.
//   voxel_route_verdict_kernel : one workgroup.  converged = no word set in the array the next round would read; it also hands the
//                                array's parity to a resuming call and reports rounds_run and n_goals_used.
//   voxel_route_finish_kernel  : one thread per cell, nothing when not converged: rule 5's direction and the three cell counts.
//   voxel_route_path_kernel    : one thread per start: a walk along the directions, a chain of dependent loads that is latency-bound
//                                by nature; bounded by d0 * d1 * d2 steps whatever the bytes hold.
//
// What passes between workgroups of one launch: halo reads of cost words that only ever fall (relaxed 32-bit loads and stores: a
// stale value is still an upper bound, and the tile that lowered it marks the reader for the next round), relaxed stores of 1 into
// the other activity array, a relaxed max for rounds_run and the counts' relaxed adds.  Every cost word is written by its own tile
// only.  No fence, no waiting on another workgroup, no persistent kernel; every loop has a bound that holds for any data.
// Bounds: a halo cell outside the volume reads cell 0 and is ignored; a tile's interior cell outside the volume is closed and is
// never written; marks go to tiles inside the tile grid only; size_t offsets (d0 * d1 * d2 reaches 2^30).
// Checks, sizes, the workspace's layout, the launch geometry and every per-cell statement are host/voxel_route.h's.
#include "kernels.h"
#include "voxel_route.h"

namespace {
typedef unsigned long long u64;
constexpr int VR_T = VOXEL_ROUTE_THREADS;

// The workspace's first VOXEL_ROUTE_HEADER_WORDS words.
enum { VR_CONVERGED = 0, VR_LAST_ACTIVE = 1, VR_PARITY = 2, VR_GOALS_USED = 3 };

struct VoxelRouteGrid {
  VoxelRouteVolume v;
  uint32_t* cost;
  uint32_t* hdr;  // the workspace
  uint32_t* act[2];
  int n0, n1, n2;  // tiles along each axis
};

struct VoxelRouteFinishArgs {
  VoxelRouteGrid g;
  size_t n;
  uint8_t* next;     // the caller's, or null
  uint8_t* ws_next;  // the workspace's, or null when no path is asked for
  u64* counts;       // or null
};

struct VoxelRoutePathArgs {
  const uint32_t* cost;
  const uint8_t* dirs;
  const uint32_t* hdr;
  const uint32_t* starts;
  uint32_t* path;
  uint32_t* path_len;
  uint8_t* path_status;
  size_t n;
  int d0, d1, d2, n_starts, max_path;
};

__device__ __forceinline__ void vr_mark(uint32_t* word) { __hip_atomic_store(word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the neighbour tile at k's offsets from (t0, t1, t2), marked if it exists
__device__ __forceinline__ void vr_mark_tile(const VoxelRouteGrid& g, uint32_t* arr, int t0, int t1, int t2, int k) {
  const int a0 = t0 + voxel_route_d0(k), a1 = t1 + voxel_route_d1(k), a2 = t2 + voxel_route_d2(k);
  if (a0 >= 0 && a0 < g.n0 && a1 >= 0 && a1 < g.n1 && a2 >= 0 && a2 < g.n2)
    vr_mark(&arr[(size_t)a0 + (size_t)g.n0 * ((size_t)a1 + (size_t)g.n1 * (size_t)a2)]);
}
}  // namespace

__global__ __launch_bounds__(VR_T) void voxel_route_goals_kernel(VoxelRouteGrid g, const uint32_t* goals, int n_goals) {
  const int i = blockIdx.x * VR_T + threadIdx.x;
  const size_t n = (size_t)g.v.d0 * (size_t)g.v.d1 * (size_t)g.v.d2;
  bool used = false;
  if (i < n_goals) {
    const uint32_t cell = goals[i];
    used = cell < n && !voxel_route_closed_bit(g.v.closed, cell);
    if (used) {
      __hip_atomic_store(&g.cost[cell], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // a duplicate stores the same word
      const uint32_t rest = cell / (uint32_t)g.v.d0;
      const int j0 = (int)(cell - rest * (uint32_t)g.v.d0), j1 = (int)(rest % (uint32_t)g.v.d1), j2 = (int)(rest / (uint32_t)g.v.d1);
      for (int k = 0; k < 27; ++k) vr_mark_tile(g, g.act[0], j0 / VOXEL_ROUTE_TX, j1 / VOXEL_ROUTE_TY, j2 / VOXEL_ROUTE_TZ, k);  // 13: its own
    }
  }
  const unsigned n_used = (unsigned)__popcll(__ballot(used));
  if ((threadIdx.x & 63) == 0 && n_used) __hip_atomic_fetch_add(&g.hdr[VR_GOALS_USED], n_used, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <int TX, int TY, int TZ>
__global__ __launch_bounds__(VR_T) void voxel_route_round_kernel(VoxelRouteGrid g, int round) {
  constexpr int P0 = TX + 2, P1 = TY + 2, P2 = TZ + 2, NP = P0 * P1 * P2, CPT = TX * TY * TZ / VR_T;
  static_assert(TX * TY * TZ % VR_T == 0 && CPT >= 1, "a tile is a whole number of cells per thread");
  __shared__ uint32_t sC[2][NP];  // cost: a sweep reads one copy and writes the other, so that one barrier per sweep is enough
  __shared__ uint32_t sQ[NP];     // 16 + pen
  __shared__ uint8_t sB[NP];      // closed, or outside the volume
  __shared__ unsigned sFaces;
  const int tid = threadIdx.x;
  const size_t tile = blockIdx.x;
  const unsigned par = (g.hdr[VR_PARITY] + (unsigned)round) & 1u;  // written by the init's memset or an earlier call's verdict only
  uint32_t* const cur = g.act[par];
  uint32_t* const nxt = g.act[par ^ 1u];
  if (cur[tile] == 0u) return;  // the same word for the whole workgroup
  if (tid == 0) sFaces = 0u;
  __syncthreads();  // every wavefront has read the word before it is cleared
  if (tid == 0) {
    cur[tile] = 0u;
    __hip_atomic_fetch_max(&g.hdr[VR_LAST_ACTIVE], (uint32_t)round + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  const size_t trest = tile / (size_t)g.n0;
  const int t0 = (int)(tile - trest * (size_t)g.n0), t1 = (int)(trest % (size_t)g.n1), t2 = (int)(trest / (size_t)g.n1);
  const int b0 = t0 * TX - 1, b1 = t1 * TY - 1, b2 = t2 * TZ - 1;
  const int d0 = g.v.d0, d1 = g.v.d1, d2 = g.v.d2;
  for (int idx = tid; idx < NP; idx += VR_T) {
    const int l2 = idx / (P0 * P1), r = idx - l2 * (P0 * P1), l1 = r / P0, l0 = r - l1 * P0;
    const int j0 = b0 + l0, j1 = b1 + l1, j2 = b2 + l2;
    const bool in = j0 >= 0 && j0 < d0 && j1 >= 0 && j1 < d1 && j2 >= 0 && j2 < d2;
    const size_t cell = in ? (size_t)j0 + (size_t)d0 * ((size_t)j1 + (size_t)d1 * (size_t)j2) : 0;  // outside: cell 0, read and ignored
    // three loads that do not wait for each other.  A halo word of cost may be written by its own tile in this very launch: a
    // relaxed load of a word that only falls.
    const bool bit = voxel_route_closed_bit(g.v.closed, cell);
    const uint32_t cc = __hip_atomic_load(&g.cost[cell], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t unit = voxel_route_unit(g.v, cell);
    const bool closed = !in || bit;
    sC[0][idx] = sC[1][idx] = closed ? VOXEL_ROUTE_NONE : cc;
    sQ[idx] = unit;
    sB[idx] = closed ? 1 : 0;
  }
  __syncthreads();
  // this thread's cells: the moves rule 2 allows out of each, what each costs (fixed for the launch), the cost on arrival and now
  int li[CPT];
  uint32_t allowed[CPT], faces[CPT], step[CPT][27], c0[CPT], c[CPT];
#pragma unroll
  for (int j = 0; j < CPT; ++j) {
    const int cidx = tid + j * VR_T, l2 = cidx / (TX * TY), r = cidx - l2 * (TX * TY), l1 = r / TX, l0 = r - l1 * TX;
    li[j] = ((l2 + 1) * P1 + l1 + 1) * P0 + l0 + 1;
    uint32_t open = 0;
#pragma unroll
    for (int k = 0; k < 27; ++k) {
      const int at = li[j] + (voxel_route_d2(k) * P1 + voxel_route_d1(k)) * P0 + voxel_route_d0(k);
      open |= sB[at] ? 0u : 1u << k;
      step[j][k] = voxel_route_weight(k) * sQ[at];  // below 2^24; [13] is not used
    }
    allowed[j] = voxel_route_allowed(open);
    faces[j] = voxel_route_faces(l0, l1, l2, TX, TY, TZ);
    c0[j] = c[j] = sC[0][li[j]];
  }
  uint32_t fallen = 0;
  bool cut_short = true, lowered = false;
  int from = 0;  // the copy this sweep reads; it writes the other one, which nobody reads before the barrier
  for (int sweep = 0; sweep < VOXEL_ROUTE_MAX_SWEEPS; ++sweep) {
    bool mine = false;
#pragma unroll
    for (int j = 0; j < CPT; ++j) {
      const uint32_t* const src = sC[from] + li[j];
      const uint32_t b = voxel_route_relax(
          c[j], allowed[j], g.v.max_cost, [&](int k) { return src[(voxel_route_d2(k) * P1 + voxel_route_d1(k)) * P0 + voxel_route_d0(k)]; },
          [&](int k) { return step[j][k]; });
      if (b < c[j]) {
        mine = true;
        fallen |= faces[j];
      }
      c[j] = b;
      sC[from ^ 1][li[j]] = b;  // every interior cell, lowered or not: the other copy is one sweep older
    }
    // the one barrier of a sweep: every read of `from` and every write of the other copy is done, and the vote is taken
    if (!__syncthreads_or(mine ? 1 : 0)) { cut_short = false; break; }
    lowered = true;
    from ^= 1;
  }
  if (!lowered) return;  // uniform: nothing to write and nobody to wake (the bound is at least one sweep, so cut_short is false)
#pragma unroll
  for (int j = 0; j < CPT; ++j)
    if (c[j] != c0[j]) {  // inside the volume and passable, or it could not have fallen
      const int cidx = tid + j * VR_T, l2 = cidx / (TX * TY), r = cidx - l2 * (TX * TY), l1 = r / TX, l0 = r - l1 * TX;
      const size_t cell = (size_t)(b0 + 1 + l0) + (size_t)d0 * ((size_t)(b1 + 1 + l1) + (size_t)d1 * (size_t)(b2 + 1 + l2));
      __hip_atomic_store(&g.cost[cell], c[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  if (fallen) atomicOr(&sFaces, fallen);
  __syncthreads();
  if (tid < 27) {
    if (tid != VOXEL_ROUTE_SELF ? ((sFaces >> tid) & 1u) != 0u : cut_short) vr_mark_tile(g, nxt, t0, t1, t2, tid);
  }
}

__global__ __launch_bounds__(VR_T) void voxel_route_verdict_kernel(uint32_t* hdr, const uint32_t* act0, const uint32_t* act1, size_t tiles,
                                                                   int max_rounds, u64* counts) {
  const unsigned par = (hdr[VR_PARITY] + (unsigned)max_rounds) & 1u;  // the array a further round would read
  const uint32_t* const arr = par ? act1 : act0;
  int any = 0;
  for (size_t t = threadIdx.x; t < tiles; t += VR_T) any |= arr[t] != 0u ? 1 : 0;
  any = __syncthreads_or(any);  // also: every thread has read the parity before it is replaced
  if (threadIdx.x == 0) {
    const uint32_t rounds = hdr[VR_LAST_ACTIVE];
    hdr[VR_CONVERGED] = any ? 0u : 1u;
    hdr[VR_LAST_ACTIVE] = 0u;
    hdr[VR_PARITY] = par;
    if (counts) {
      counts[0] = hdr[VR_GOALS_USED];
      counts[4] = any ? 0u : 1u;
      counts[5] = rounds;
    }
  }
}

__global__ __launch_bounds__(VR_T) void voxel_route_finish_kernel(VoxelRouteFinishArgs a) {
  __shared__ unsigned sN[3][VR_T / 64];
  if (a.g.hdr[VR_CONVERGED] == 0u) return;  // uniform over the launch
  const int tid = threadIdx.x;
  const size_t i = (size_t)blockIdx.x * VR_T + (size_t)tid;
  unsigned n_reached = 0, n_unreached = 0, n_closed = 0;
  if (i < a.n) {
    const uint8_t dir = voxel_route_next_one(a.g.v, a.g.cost, i);
    const bool closed = voxel_route_closed_bit(a.g.v.closed, i), none = a.g.cost[i] == VOXEL_ROUTE_NONE;
    if (a.next) a.next[i] = dir;
    if (a.ws_next) a.ws_next[i] = dir;
    n_closed = closed ? 1u : 0u;
    n_reached = !closed && !none ? 1u : 0u;
    n_unreached = !closed && none ? 1u : 0u;
  }
  if (!a.counts) return;  // uniform over the launch
  for (int o = 32; o > 0; o >>= 1) {
    n_reached += __shfl_xor(n_reached, o);
    n_unreached += __shfl_xor(n_unreached, o);
    n_closed += __shfl_xor(n_closed, o);
  }
  if ((tid & 63) == 0) { sN[0][tid >> 6] = n_reached; sN[1][tid >> 6] = n_unreached; sN[2][tid >> 6] = n_closed; }
  __syncthreads();
  if (tid < 3) {
    unsigned t = 0;
    for (int w = 0; w < VR_T / 64; ++w) t += sN[tid][w];
    if (t) __hip_atomic_fetch_add(&a.counts[1 + tid], (u64)t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__global__ __launch_bounds__(VR_T) void voxel_route_path_kernel(VoxelRoutePathArgs a) {
  const int i = blockIdx.x * VR_T + threadIdx.x;
  if (i >= a.n_starts) return;
  uint32_t len = 0;
  uint8_t status = VOXEL_ROUTE_NOT_CONVERGED;
  if (a.hdr[VR_CONVERGED] != 0u) {
    const uint32_t s = a.starts[i];
    if (s >= a.n) status = VOXEL_ROUTE_OUT_OF_VOLUME;
    else if (a.cost[s] == VOXEL_ROUTE_NONE) status = VOXEL_ROUTE_UNREACHED;
    else {
      uint32_t* const row = a.path + (size_t)i * (size_t)a.max_path;
      uint32_t v = s;
      // each step's byte names the next cell to read: dependent loads, latency-bound by nature.  A route visits a cell once, so
      // d0 * d1 * d2 steps bound it whatever the bytes hold; a byte that leaves the volume or is no move ends the walk.
      for (size_t step = 0; step < a.n; ++step) {
        if (len < (uint32_t)a.max_path) row[len] = v;
        ++len;
        v = voxel_route_step(v, a.dirs[v], a.d0, a.d1, a.d2);
        if (v == VOXEL_ROUTE_NONE) break;
      }
      status = len > (uint32_t)a.max_path ? VOXEL_ROUTE_TRUNCATED : VOXEL_ROUTE_OK;
    }
  }
  a.path_len[i] = len;
  a.path_status[i] = status;
}

// ----------------------------------------------------------------------------- host side
extern "C" int svo_voxel_route_default_params(float voxel_size, svo_voxel_route_params* out) { return voxel_route_default_params(voxel_size, out); }
extern "C" int svo_voxel_route_workspace_bytes(const int* dims3, size_t* bytes) { return voxel_route_workspace_bytes(dims3, bytes); }
extern "C" int svo_voxel_occupancy_cell_of(float voxel_size, const int* origin3, const int* dims3, const float* xyz3, uint32_t* cell) {
  return voxel_occupancy_cell_of(voxel_size, origin3, dims3, xyz3, cell);
}

extern "C" int svo_voxel_occupancy_route_dev(svo_voxel_map* m, const uint64_t* closed, const int* dims3, const uint16_t* dist2,
                                             const svo_voxel_route_params* prm, const uint32_t* goals, int n_goals, const uint32_t* starts,
                                             int n_starts, void* workspace, const svo_voxel_route_out* out, uint64_t* counts) {
  if (!m) return SVO_ERR_INVALID;
  const SvoVoxelView t = svo_voxel_map_view(m);
  svo_ctx* ctx = t.ctx;
  svo_use_device(ctx);
  SVO_ARGS_CHECK(ctx, voxel_route_check(closed, dims3, dist2, prm, goals, n_goals, starts, n_starts, workspace, out, counts, &err));
  unsigned char* const ws = static_cast<unsigned char*>(workspace);
  const VoxelRouteTiles tiles = voxel_route_tiles(dims3);
  VoxelRouteGrid g{};
  g.v.closed = closed; g.v.dist2 = dist2;
  g.v.d0 = dims3[0]; g.v.d1 = dims3[1]; g.v.d2 = dims3[2];
  g.v.near_r2 = prm->near_r2; g.v.near_weight = prm->near_weight; g.v.max_cost = prm->max_cost;
  g.cost = out->cost;
  g.hdr = reinterpret_cast<uint32_t*>(ws);
  g.act[0] = reinterpret_cast<uint32_t*>(ws + voxel_route_ws_activity_offset(0, dims3));
  g.act[1] = reinterpret_cast<uint32_t*>(ws + voxel_route_ws_activity_offset(1, dims3));
  g.n0 = (int)tiles.n0; g.n1 = (int)tiles.n1; g.n2 = (int)tiles.n2;
  const size_t n = voxel_distance_cells(dims3), o_next = voxel_route_ws_next_offset(dims3);
  const bool paths = n_starts > 0 && out->path;
  u64* const d_counts = reinterpret_cast<u64*>(counts);
  hipStream_t st = ctx->stream;
  SvoProfScope prof(ctx, SVO_PROF_VOXEL_ROUTE);
  if (counts) SVO_HIP_CHECK(ctx, hipMemsetAsync(counts, 0, 8 * sizeof(u64), st));
  if (!prm->resume) {
    SVO_HIP_CHECK(ctx, hipMemsetAsync(out->cost, 0xFF, 4 * n, st));  // NONE everywhere
    SVO_HIP_CHECK(ctx, hipMemsetAsync(ws, 0, o_next, st));           // the header and both activity arrays
    hipLaunchKernelGGL(voxel_route_goals_kernel, dim3((unsigned)voxel_route_groups((size_t)n_goals)), dim3(VR_T), 0, st, g, goals, n_goals);
    SVO_HIP_CHECK(ctx, hipGetLastError());
  }
  for (int round = 0; round < prm->max_rounds; ++round) {
    hipLaunchKernelGGL((voxel_route_round_kernel<VOXEL_ROUTE_TX, VOXEL_ROUTE_TY, VOXEL_ROUTE_TZ>), dim3((unsigned)tiles.total), dim3(VR_T), 0, st, g, round);
    SVO_HIP_CHECK(ctx, hipGetLastError());
  }
  hipLaunchKernelGGL(voxel_route_verdict_kernel, dim3(1), dim3(VR_T), 0, st, g.hdr, g.act[0], g.act[1], tiles.total, prm->max_rounds, d_counts);
  SVO_HIP_CHECK(ctx, hipGetLastError());
  if (out->next || counts || paths) {
    VoxelRouteFinishArgs f{};
    f.g = g; f.n = n;
    f.next = out->next;
    f.ws_next = paths ? ws + o_next : nullptr;
    f.counts = d_counts;
    hipLaunchKernelGGL(voxel_route_finish_kernel, dim3((unsigned)voxel_route_groups(n)), dim3(VR_T), 0, st, f);
    SVO_HIP_CHECK(ctx, hipGetLastError());
  }
  if (paths) {
    VoxelRoutePathArgs p{};
    p.cost = out->cost; p.dirs = ws + o_next; p.hdr = g.hdr; p.starts = starts;
    p.path = out->path; p.path_len = out->path_len; p.path_status = out->path_status;
    p.n = n; p.d0 = dims3[0]; p.d1 = dims3[1]; p.d2 = dims3[2]; p.n_starts = n_starts; p.max_path = prm->max_path;
    hipLaunchKernelGGL(voxel_route_path_kernel, dim3((unsigned)voxel_route_groups((size_t)n_starts)), dim3(VR_T), 0, st, p);
    SVO_HIP_CHECK(ctx, hipGetLastError());
  }
  return SVO_OK;
}

extern "C" int svo_voxel_occupancy_route(svo_voxel_map* m, const uint64_t* closed, const int* dims3, const uint16_t* dist2,
                                         const svo_voxel_route_params* prm, const uint32_t* goals, int n_goals, const uint32_t* starts,
                                         int n_starts, const svo_voxel_route_out* out, uint64_t* counts) {
  if (!m) return SVO_ERR_INVALID;
  const SvoVoxelView t = svo_voxel_map_view(m);
  svo_ctx* ctx = t.ctx;
  svo_use_device(ctx);
  SVO_ARGS_CHECK(ctx, voxel_route_host_check(closed, dims3, dist2, prm, goals, n_goals, starts, n_starts, out, &err));
  size_t b_ws = 0;
  (void)voxel_route_workspace_bytes(dims3, &b_ws);
  const size_t n = voxel_distance_cells(dims3), ns = (size_t)n_starts, ng = (size_t)n_goals;
  const bool paths = ns > 0 && out->path;
  const size_t b_path = paths ? 4 * ns * (size_t)prm->max_path : 0;
  SvoParts parts;
  const size_t o_counts = parts.add(8 * sizeof(u64)), o_ws = parts.add(b_ws), o_cost = parts.add(4 * n), o_goals = parts.add(4 * ng),
               o_starts = parts.add(4 * ns), o_len = parts.add(4 * ns), o_path = parts.add(b_path), o_next = parts.add(out->next ? n : 0),
               o_status = parts.add(ns);
  SvoTemp d;
  SVO_HIP_CHECK(ctx, hipMalloc(&d.p, parts.total()));
  svo_voxel_route_out o{};
  o.cost = d.at<uint32_t>(o_cost);
  o.next = out->next ? d.at(o_next) : nullptr;  // what the caller did not ask for is not written
  if (paths) { o.path = d.at<uint32_t>(o_path); o.path_len = d.at<uint32_t>(o_len); o.path_status = d.at(o_status); }
  u64 c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  hipStream_t st = ctx->stream;
  // The caller's next and path go up first, so that what the contract leaves untouched comes back as it was.
  hipError_t e = hipMemcpyAsync(d.at(o_goals), goals, 4 * ng, hipMemcpyHostToDevice, st);
  if (e == hipSuccess && ns) e = hipMemcpyAsync(d.at(o_starts), starts, 4 * ns, hipMemcpyHostToDevice, st);
  if (e == hipSuccess && out->next) e = hipMemcpyAsync(o.next, out->next, n, hipMemcpyHostToDevice, st);
  if (e == hipSuccess && paths) e = hipMemcpyAsync(o.path, out->path, b_path, hipMemcpyHostToDevice, st);
  const int rc = svo_host_call(
      ctx, "voxel_route", e,
      [&] {
        return svo_voxel_occupancy_route_dev(m, closed, dims3, dist2, prm, d.at<uint32_t>(o_goals), n_goals, ns ? d.at<uint32_t>(o_starts) : nullptr,
                                             n_starts, d.at(o_ws), &o, d.at<uint64_t>(o_counts));
      },
      [&] {
        hipError_t e = hipMemcpyAsync(out->cost, o.cost, 4 * n, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && out->next) e = hipMemcpyAsync(out->next, o.next, n, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && paths) e = hipMemcpyAsync(out->path, o.path, b_path, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && paths) e = hipMemcpyAsync(out->path_len, o.path_len, 4 * ns, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && paths) e = hipMemcpyAsync(out->path_status, o.path_status, ns, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(c, d.at(o_counts), sizeof(c), hipMemcpyDeviceToHost, st);
        return e;
      });
  if (rc) return rc;
  if (counts) for (int k = 0; k < 8; ++k) counts[k] = c[k];
  return SVO_OK;
}
