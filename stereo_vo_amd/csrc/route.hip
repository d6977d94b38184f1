// Ground plan route (include/svo.h, "Ground plan route"): the cost-to-go field to goal cells over a u8 grid, the first
// move per cell and the paths from start cells, on the context's stream.  A Bellman-Ford fixed point with positive integer weights is
// unique whatever the order of relaxation, so the tiled form below gives Dijkstra's field bit for bit once it has converged.
//
//   route_goals_kernel   : one thread per goal entry (after the memsets that set cost to NONE and zero the workspace's header and
//                          activity words).  A used goal gets cost 0 and marks its tile and the eight around it in activity array 0.
//   route_round_kernel   : enqueued max_rounds times, one workgroup per T x T tile.  A tile whose word in this round's activity
//                          array is 0 exits.  An active one clears the word, loads cost, blocked and 16 + pen with a one-cell halo
//                          into LDS and sweeps: every cell takes the minimum over its allowed moves, read from one copy of the
//                          tile and written to a second one, a barrier, the copies swapped, until a sweep changes nothing or
//                          ROUTE_MAX_SWEEPS are done.  It then writes the
//                          lowered cells back, marks in the OTHER array the neighbours whose halo saw a border cell change, and
//                          itself if the sweep bound cut it short.
//   route_verdict_kernel : one workgroup.  converged = no word set in the array the next round would read; it also hands the
//                          array's parity to a resuming call and reports rounds_run and n_goals_used.
//   route_finish_kernel  : one thread per cell, nothing when not converged: rule 5's direction and the three cell counts.
//   route_path_kernel    : one thread per start: a walk along the directions, a chain of dependent loads that is latency-bound by
//                          nature (one byte, then the next cell's byte); bounded by na * nb steps whatever the bytes hold.
//
// What passes between workgroups of one launch: halo reads of cost words that only ever fall (relaxed 32-bit loads and stores: a
// stale value is still an upper bound, and the tile that lowered it marks the reader for the next round), relaxed stores of 1 into
// the other activity array, a relaxed max for rounds_run and the counts' relaxed adds.  Every cost word is written by its own tile
// only.  No fence, no waiting on another workgroup, no persistent kernel; every loop has a bound that holds for any data.
// Checks, sizes, the workspace's layout and the launch geometry are host/route_args.h's.
#include "route_args.h"
#include "kernels.h"

namespace {
using u64 = unsigned long long;
constexpr int RT_T = ROUTE_THREADS;

// The workspace's first ROUTE_HEADER_WORDS words.
enum { RT_CONVERGED = 0, RT_LAST_ACTIVE = 1, RT_PARITY = 2, RT_GOALS_USED = 3 };

struct RouteGrid {
  const uint8_t* blocked;
  const uint32_t* dist2;  // or null
  uint32_t* cost;
  uint32_t* hdr;          // the workspace
  uint32_t* act[2];
  int na, nb, ta, tb;     // cells and tiles either way
  uint32_t near_r2, near_weight, max_cost;
};

struct RouteFinishArgs {
  RouteGrid g;
  size_t n;
  uint8_t* next;     // the caller's, or null
  uint8_t* ws_next;  // the workspace's, or null when no path is asked for
  u64* counts;       // or null
};

struct RoutePathArgs {
  const uint32_t* cost;
  const uint8_t* dirs;
  const uint32_t* hdr;
  const uint32_t* starts;
  uint32_t* path;
  uint32_t* path_len;
  uint8_t* path_status;
  size_t n;
  int nb, na, n_starts, max_path;
};

__device__ __forceinline__ int rt_dia(int k) { return k < 3 ? -1 : (k < 5 ? 0 : 1); }
__device__ __forceinline__ int rt_dib(int k) { return k < 3 ? k - 1 : (k == 3 ? -1 : (k == 4 ? 1 : k - 6)); }
__device__ __forceinline__ uint32_t rt_weight(int k) { return (k == 1 || k == 3 || k == 4 || k == 6) ? 5u : 7u; }
// rule 1 plus the chamfer's unit: what a move INTO the cell costs per unit of w
__device__ __forceinline__ uint32_t rt_unit(const RouteGrid& g, size_t cell) {
  if (!g.dist2) return 16u;
  const uint32_t d = g.dist2[cell];
  return 16u + (d < g.near_r2 ? g.near_weight * (g.near_r2 - d) : 0u);
}
__device__ __forceinline__ void rt_mark(uint32_t* word) { __hip_atomic_store(word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
}  // namespace

__global__ __launch_bounds__(RT_T) void route_goals_kernel(RouteGrid g, const uint32_t* goals, int n_goals) {
  const int i = blockIdx.x * RT_T + threadIdx.x;
  const size_t n = (size_t)g.na * (size_t)g.nb;
  bool used = false;
  if (i < n_goals) {
    const uint32_t cell = goals[i];
    used = cell < n && g.blocked[cell] == 0;
    if (used) {
      __hip_atomic_store(&g.cost[cell], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // a duplicate stores the same word
      const int ia = (int)(cell / (uint32_t)g.nb), ib = (int)(cell - (uint32_t)ia * (uint32_t)g.nb);
      const int tia = ia / ROUTE_TILE, tib = ib / ROUTE_TILE;
      for (int da = -1; da <= 1; ++da)
        for (int db = -1; db <= 1; ++db) {
          const int a = tia + da, b = tib + db;
          if (a >= 0 && a < g.ta && b >= 0 && b < g.tb) rt_mark(&g.act[0][(size_t)a * (size_t)g.tb + (size_t)b]);
        }
    }
  }
  const unsigned n_used = (unsigned)__popcll(__ballot(used));
  if ((threadIdx.x & 63) == 0 && n_used) __hip_atomic_fetch_add(&g.hdr[RT_GOALS_USED], n_used, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <int T>
__global__ __launch_bounds__(RT_T) void route_round_kernel(RouteGrid g, int round) {
  constexpr int P = T + 2, CPT = T * T / RT_T;
  static_assert(T * T % RT_T == 0 && CPT >= 1, "a tile is a whole number of cells per thread");
  __shared__ uint32_t sC[2][P * P];  // cost: a sweep reads one copy and writes the other, so that one barrier per sweep is enough
  __shared__ uint32_t sQ[P * P];     // 16 + pen
  __shared__ uint8_t sB[P * P];      // impassable, or outside the grid
  __shared__ unsigned sDirs;
  const int tid = threadIdx.x;
  const size_t tile = blockIdx.x;
  const unsigned par = (g.hdr[RT_PARITY] + (unsigned)round) & 1u;  // written by the init's memset or an earlier call's verdict only
  uint32_t* const cur = g.act[par];
  uint32_t* const nxt = g.act[par ^ 1u];
  if (cur[tile] == 0u) return;  // the same word for the whole workgroup
  if (tid == 0) sDirs = 0u;
  __syncthreads();  // every wavefront has read the word before it is cleared
  if (tid == 0) {
    cur[tile] = 0u;
    __hip_atomic_fetch_max(&g.hdr[RT_LAST_ACTIVE], (uint32_t)round + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  const int tia = (int)(tile / (size_t)g.tb), tib = (int)(tile - (size_t)tia * (size_t)g.tb);
  const int a0 = tia * T - 1, b0 = tib * T - 1;
  for (int idx = tid; idx < P * P; idx += RT_T) {
    const int ly = idx / P, lx = idx - ly * P;
    const int ga = a0 + ly, gb = b0 + lx;
    const bool in = ga >= 0 && ga < g.na && gb >= 0 && gb < g.nb;
    const size_t cell = in ? (size_t)ga * (size_t)g.nb + (size_t)gb : 0;  // outside the grid: cell 0, read and ignored
    // three loads that do not wait for each other.  A halo word of cost may be written by its own tile in this very launch: a
    // relaxed load of a word that only falls.
    const uint8_t bl = g.blocked[cell];
    const uint32_t cc = __hip_atomic_load(&g.cost[cell], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t unit = rt_unit(g, cell);
    const bool closed = !in || bl != 0;
    sC[0][idx] = sC[1][idx] = closed ? ROUTE_NONE : cc;
    sQ[idx] = unit;
    sB[idx] = closed ? 1 : 0;
  }
  __syncthreads();
  // this thread's cells: what each move rule 2 allows out of it costs (fixed for the launch), the cost on arrival and now
  int li[CPT];
  unsigned allowed[CPT], edge[CPT];
  uint32_t step[CPT][8], c0[CPT], c[CPT];
#pragma unroll
  for (int j = 0; j < CPT; ++j) {
    const int cidx = tid + j * RT_T, ly = cidx / T, lx = cidx - ly * T;
    li[j] = (ly + 1) * P + lx + 1;
    unsigned m = 0;
    const bool open = !sB[li[j]];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int da = rt_dia(k), db = rt_dib(k);
      const bool ok = open && !sB[li[j] + da * P + db] && (da == 0 || db == 0 || (!sB[li[j] + da * P] && !sB[li[j] + db]));
      m |= ok ? 1u << k : 0u;
      step[j][k] = rt_weight(k) * sQ[li[j] + da * P + db];  // less than 2^23
    }
    allowed[j] = m;
    const bool n_ = ly == 0, s_ = ly == T - 1, w_ = lx == 0, e_ = lx == T - 1;
    edge[j] = (n_ && w_ ? 1u : 0u) | (n_ ? 2u : 0u) | (n_ && e_ ? 4u : 0u) | (w_ ? 8u : 0u) | (e_ ? 16u : 0u) | (s_ && w_ ? 32u : 0u) |
              (s_ ? 64u : 0u) | (s_ && e_ ? 128u : 0u);
    c0[j] = c[j] = sC[0][li[j]];
  }
  unsigned dirs = 0;
  bool cut_short = true, lowered = false;
  int from = 0;  // the copy this sweep reads; it writes the other one, which nobody reads before the barrier
  for (int sweep = 0; sweep < ROUTE_MAX_SWEEPS; ++sweep) {
    bool mine = false;
#pragma unroll
    for (int j = 0; j < CPT; ++j) {
      uint32_t b = c[j];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const uint32_t cu = sC[from][li[j] + rt_dia(k) * P + rt_dib(k)];
        const uint32_t cand = cu + step[j][k];  // looked at only where cu is a cost: at most 0x7F000000 + 2^23
        const bool ok = ((allowed[j] >> k) & 1u) != 0u && cu != ROUTE_NONE && cand <= g.max_cost;
        b = ok && cand < b ? cand : b;
      }
      if (b < c[j]) {
        mine = true;
        dirs |= edge[j];
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
    if (c[j] != c0[j]) {  // inside the grid and passable, or it could not have fallen
      const int cidx = tid + j * RT_T, ly = cidx / T, lx = cidx - ly * T;
      const size_t cell = (size_t)(a0 + 1 + ly) * (size_t)g.nb + (size_t)(b0 + 1 + lx);
      __hip_atomic_store(&g.cost[cell], c[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  if (dirs) atomicOr(&sDirs, dirs);
  __syncthreads();
  if (tid < 8) {
    const int a = tia + rt_dia(tid), b = tib + rt_dib(tid);
    if (((sDirs >> tid) & 1u) != 0u && a >= 0 && a < g.ta && b >= 0 && b < g.tb) rt_mark(&nxt[(size_t)a * (size_t)g.tb + (size_t)b]);
  } else if (tid == 8 && cut_short) {
    rt_mark(&nxt[tile]);
  }
}

__global__ __launch_bounds__(RT_T) void route_verdict_kernel(uint32_t* hdr, const uint32_t* act0, const uint32_t* act1, size_t tiles,
                                                             int max_rounds, u64* counts) {
  const unsigned par = (hdr[RT_PARITY] + (unsigned)max_rounds) & 1u;  // the array a further round would read
  const uint32_t* const arr = par ? act1 : act0;
  int any = 0;
  for (size_t t = threadIdx.x; t < tiles; t += RT_T) any |= arr[t] != 0u ? 1 : 0;
  any = __syncthreads_or(any);  // also: every thread has read the parity before it is replaced
  if (threadIdx.x == 0) {
    const uint32_t rounds = hdr[RT_LAST_ACTIVE];
    hdr[RT_CONVERGED] = any ? 0u : 1u;
    hdr[RT_LAST_ACTIVE] = 0u;
    hdr[RT_PARITY] = par;
    if (counts) {
      counts[0] = hdr[RT_GOALS_USED];
      counts[4] = any ? 0u : 1u;
      counts[5] = rounds;
    }
  }
}

__global__ __launch_bounds__(RT_T) void route_finish_kernel(RouteFinishArgs a) {
  __shared__ unsigned sN[3][RT_T / 64];
  if (a.g.hdr[RT_CONVERGED] == 0u) return;  // uniform over the launch
  const RouteGrid& g = a.g;
  const int tid = threadIdx.x;
  const size_t i = (size_t)blockIdx.x * RT_T + (size_t)tid;
  unsigned n_reached = 0, n_unreached = 0, n_closed = 0;
  if (i < a.n) {
    const int nb = g.nb, na = g.na;
    const int ia = (int)(i / (size_t)nb), ib = (int)(i - (size_t)ia * (size_t)nb);
    const uint32_t c = g.cost[i];
    const bool closed = g.blocked[i] != 0;
    uint8_t dir = 255;
    if (c == 0u) dir = 8;
    else if (c != ROUTE_NONE) {
      for (int k = 7; k >= 0; --k) {  // downward, so that the smallest k stays
        const int ja = ia + rt_dia(k), jb = ib + rt_dib(k);
        if (ja < 0 || ja >= na || jb < 0 || jb >= nb) continue;
        const size_t u = (size_t)ja * (size_t)nb + (size_t)jb;
        if (g.blocked[u] != 0) continue;
        if (ja != ia && jb != ib && (g.blocked[(size_t)ja * (size_t)nb + (size_t)ib] != 0 || g.blocked[(size_t)ia * (size_t)nb + (size_t)jb] != 0)) continue;
        const uint32_t cu = g.cost[u];
        if (cu != ROUTE_NONE && cu + rt_weight(k) * rt_unit(g, u) == c) dir = (uint8_t)k;
      }
    }
    if (a.next) a.next[i] = dir;
    if (a.ws_next) a.ws_next[i] = dir;
    n_closed = closed ? 1u : 0u;
    n_reached = !closed && c != ROUTE_NONE ? 1u : 0u;
    n_unreached = !closed && c == ROUTE_NONE ? 1u : 0u;
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
    for (int w = 0; w < RT_T / 64; ++w) t += sN[tid][w];
    if (t) __hip_atomic_fetch_add(&a.counts[1 + tid], (u64)t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__global__ __launch_bounds__(RT_T) void route_path_kernel(RoutePathArgs a) {
  const int i = blockIdx.x * RT_T + threadIdx.x;
  if (i >= a.n_starts) return;
  uint32_t len = 0;
  uint8_t status = SVO_GRID_ROUTE_NOT_CONVERGED;
  if (a.hdr[RT_CONVERGED] != 0u) {
    const uint32_t s = a.starts[i];
    if (s >= a.n) status = SVO_GRID_ROUTE_OUT_OF_GRID;
    else if (a.cost[s] == ROUTE_NONE) status = SVO_GRID_ROUTE_UNREACHED;
    else {
      uint32_t* const row = a.path + (size_t)i * (size_t)a.max_path;
      uint32_t v = s;
      // each step's byte names the next cell to read: dependent loads, latency-bound by nature.  A route visits a cell once, so
      // na * nb steps bound it whatever the bytes hold; a byte that leaves the grid or is no direction ends the walk.
      for (size_t step = 0; step < a.n; ++step) {
        if (len < (uint32_t)a.max_path) row[len] = v;
        ++len;
        const unsigned k = a.dirs[v];
        if (k >= 8u) break;
        const int ia = (int)(v / (uint32_t)a.nb), ib = (int)(v - (uint32_t)ia * (uint32_t)a.nb);
        const int ja = ia + rt_dia((int)k), jb = ib + rt_dib((int)k);
        if (ja < 0 || ja >= a.na || jb < 0 || jb >= a.nb) break;
        v = (uint32_t)ja * (uint32_t)a.nb + (uint32_t)jb;
      }
      status = len > (uint32_t)a.max_path ? SVO_GRID_ROUTE_TRUNCATED : SVO_GRID_ROUTE_OK;
    }
  }
  a.path_len[i] = len;
  a.path_status[i] = status;
}

// ----------------------------------------------------------------------------- host side
extern "C" int svo_grid_route_default_params(const svo_grid_clearance_params* clearance, svo_grid_route_params* out) {
  return route_default_params(clearance, out);
}

extern "C" size_t svo_grid_route_workspace_bytes(int na, int nb) { return route_workspace_bytes(na, nb); }

extern "C" int svo_grid_route_dev(svo_ctx* ctx, const uint8_t* blocked, const uint32_t* dist2, const svo_grid_route_params* prm,
                                  const uint32_t* goals, int n_goals, const uint32_t* starts, int n_starts, void* workspace,
                                  const svo_grid_route_out* out, uint64_t* counts) {
  if (!ctx) return SVO_ERR_INVALID;
  svo_use_device(ctx);
  SVO_ARGS_CHECK(ctx, route_check(blocked, dist2, prm, goals, n_goals, starts, n_starts, workspace, out, counts, &err));
  const int na = prm->na, nb = prm->nb;
  unsigned char* const ws = static_cast<unsigned char*>(workspace);
  RouteGrid g{};
  g.blocked = blocked; g.dist2 = dist2; g.cost = out->cost;
  g.hdr = reinterpret_cast<uint32_t*>(ws);
  g.act[0] = reinterpret_cast<uint32_t*>(ws + route_ws_activity_offset(0, na, nb));
  g.act[1] = reinterpret_cast<uint32_t*>(ws + route_ws_activity_offset(1, na, nb));
  g.na = na; g.nb = nb; g.ta = (int)route_tiles_along(na); g.tb = (int)route_tiles_along(nb);
  g.near_r2 = prm->near_r2; g.near_weight = prm->near_weight; g.max_cost = prm->max_cost;
  const size_t n = (size_t)na * (size_t)nb, tiles = route_tiles(na, nb);
  const bool paths = n_starts > 0 && out->path;
  u64* const d_counts = reinterpret_cast<u64*>(counts);
  hipStream_t st = ctx->stream;
  SvoProfScope prof(ctx, SVO_PROF_GRID_ROUTE);
  if (counts) SVO_HIP_CHECK(ctx, hipMemsetAsync(counts, 0, 8 * sizeof(u64), st));
  if (!prm->resume) {
    SVO_HIP_CHECK(ctx, hipMemsetAsync(out->cost, 0xFF, 4 * n, st));                  // NONE everywhere
    SVO_HIP_CHECK(ctx, hipMemsetAsync(ws, 0, route_ws_next_offset(na, nb), st));      // the header and both activity arrays
    hipLaunchKernelGGL(route_goals_kernel, dim3((unsigned)route_groups((size_t)n_goals)), dim3(RT_T), 0, st, g, goals, n_goals);
    SVO_HIP_CHECK(ctx, hipGetLastError());
  }
  for (int round = 0; round < prm->max_rounds; ++round) {
    hipLaunchKernelGGL(route_round_kernel<ROUTE_TILE>, dim3((unsigned)tiles), dim3(RT_T), 0, st, g, round);
    SVO_HIP_CHECK(ctx, hipGetLastError());
  }
  hipLaunchKernelGGL(route_verdict_kernel, dim3(1), dim3(RT_T), 0, st, g.hdr, g.act[0], g.act[1], tiles, prm->max_rounds, d_counts);
  SVO_HIP_CHECK(ctx, hipGetLastError());
  if (out->next || counts || paths) {
    RouteFinishArgs f{};
    f.g = g; f.n = n;
    f.next = out->next;
    f.ws_next = paths ? ws + route_ws_next_offset(na, nb) : nullptr;
    f.counts = d_counts;
    hipLaunchKernelGGL(route_finish_kernel, dim3((unsigned)route_groups(n)), dim3(RT_T), 0, st, f);
    SVO_HIP_CHECK(ctx, hipGetLastError());
  }
  if (paths) {
    RoutePathArgs p{};
    p.cost = out->cost; p.dirs = ws + route_ws_next_offset(na, nb); p.hdr = g.hdr; p.starts = starts;
    p.path = out->path; p.path_len = out->path_len; p.path_status = out->path_status;
    p.n = n; p.nb = nb; p.na = na; p.n_starts = n_starts; p.max_path = prm->max_path;
    hipLaunchKernelGGL(route_path_kernel, dim3((unsigned)route_groups((size_t)n_starts)), dim3(RT_T), 0, st, p);
    SVO_HIP_CHECK(ctx, hipGetLastError());
  }
  return SVO_OK;
}

extern "C" int svo_grid_route(svo_ctx* ctx, const uint8_t* blocked, const uint32_t* dist2, const svo_grid_route_params* prm,
                              const uint32_t* goals, int n_goals, const uint32_t* starts, int n_starts, const svo_grid_route_out* out,
                              uint64_t* counts) {
  if (!ctx) return SVO_ERR_INVALID;
  svo_use_device(ctx);
  SVO_REQUIRE(ctx, blocked, "grid_route: null blocked");
  SVO_ARGS_CHECK(ctx, route_params_check(prm, n_starts, &err));
  SVO_REQUIRE(ctx, prm->resume == 0, "grid_route: resume needs the _dev entry, whose workspace outlives the call");
  SVO_ARGS_CHECK(ctx, route_lists_check(goals, n_goals, starts, n_starts, &err));
  SVO_ARGS_CHECK(ctx, route_out_check(out, n_starts, false, &err));
  const size_t n = (size_t)prm->na * (size_t)prm->nb, ns = (size_t)n_starts, ng = (size_t)n_goals;
  const bool paths = ns > 0 && out->path;
  const size_t b_path = paths ? 4 * ns * (size_t)prm->max_path : 0;
  SvoParts parts;
  const size_t o_counts = parts.add(8 * sizeof(u64)), o_ws = parts.add(route_workspace_bytes(prm->na, prm->nb)), o_cost = parts.add(4 * n),
               o_d2 = parts.add(4 * n), o_goals = parts.add(4 * ng), o_starts = parts.add(4 * ns), o_len = parts.add(4 * ns),
               o_path = parts.add(b_path), o_next = parts.add(n), o_blocked = parts.add(n), o_status = parts.add(ns);
  SvoTemp d;
  SVO_HIP_CHECK(ctx, hipMalloc(&d.p, parts.total()));
  svo_grid_route_out o{};
  o.cost = d.at<uint32_t>(o_cost);
  o.next = out->next ? d.at(o_next) : nullptr;  // what the caller did not ask for is not written
  if (paths) { o.path = d.at<uint32_t>(o_path); o.path_len = d.at<uint32_t>(o_len); o.path_status = d.at(o_status); }
  u64 c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  hipStream_t st = ctx->stream;
  // The caller's next and path go up first, so that what the contract leaves untouched comes back as it was.
  hipError_t e = hipMemcpyAsync(d.at(o_blocked), blocked, n, hipMemcpyHostToDevice, st);
  if (e == hipSuccess && dist2) e = hipMemcpyAsync(d.at(o_d2), dist2, 4 * n, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d.at(o_goals), goals, 4 * ng, hipMemcpyHostToDevice, st);
  if (e == hipSuccess && ns) e = hipMemcpyAsync(d.at(o_starts), starts, 4 * ns, hipMemcpyHostToDevice, st);
  if (e == hipSuccess && out->next) e = hipMemcpyAsync(o.next, out->next, n, hipMemcpyHostToDevice, st);
  if (e == hipSuccess && paths) e = hipMemcpyAsync(o.path, out->path, b_path, hipMemcpyHostToDevice, st);
  const int rc = svo_host_call(
      ctx, "grid_route", e,
      [&] {
        return svo_grid_route_dev(ctx, d.at(o_blocked), dist2 ? d.at<uint32_t>(o_d2) : nullptr, prm, d.at<uint32_t>(o_goals), n_goals,
                                  ns ? d.at<uint32_t>(o_starts) : nullptr, n_starts, d.at(o_ws), &o, d.at<uint64_t>(o_counts));
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
