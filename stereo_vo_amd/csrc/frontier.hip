// Ground plan frontiers (include/svo.h, "Ground plan frontiers"): the FREE cells of a u8 class grid that touch an
// UNKNOWN cell along an edge, grouped into 8-connected components, each with its size, bounds, sums, representative and cheapest
// cell, ranked by smallest cell index, on the context's stream.  Connected-component labelling by union-find as in speckle.hip; ten
// launches:
//
//   frontier_tile_kernel   : one workgroup per 16 x 16 tile.  Classifies the cells (rules 1-2) from a one-cell halo of cls in LDS, runs
//                            an 8-connected union-find in LDS, writes per cell parent = the cell index of its tile-local root (NONE
//                            for a cell that is no frontier cell) and size = the tile-local component's size at its root, 0 elsewhere;
//                            adds the three cell tallies once per workgroup.
//   frontier_seam_kernel   : one thread per cell on the far side of a tile seam: unite with the three neighbours across the seam by
//                            speckle_seam_kernel's bounded atomicMin hook loop.  The root of a frontier is then its smallest cell.
//   frontier_size_kernel   : every tile-local root that is no longer a root adds its size to its root's: one atomic per tile-local
//                            component; it then puts itself directly under that root, so that the chain of seam hooks is walked once
//                            per tile-local root and every later find takes two steps.
//   frontier_count_kernel  : per block of 256 cells the number of kept roots (parent == cell, size >= min_size); the three frontier
//                            tallies.
//   frontier_scan_kernel   : one workgroup turns the block counts into exclusive prefixes in a loop of 256 at a time; n_kept.
//   frontier_rank_kernel   : rank = block prefix + prefix within the block at every kept root, NONE elsewhere; a kept root of rank <
//                            max_frontiers initialises its slot of the statistics table.
//   frontier_stats_kernel  : every frontier cell finds its root and takes its rank (written to label and kept per cell); cells of rank
//                            < max_frontiers add into their slot: sums, bounds and the cheapest cell.  Runs of equal rank along the
//                            lanes of a wavefront are combined by a segmented shuffle reduction first, so that a run costs the seven
//                            atomics once, not once per cell (svo_grid_frontier_set_mode turns that off for the measurement).
//   frontier_centroid_kernel: one thread per written slot: the floored centroid.
//   frontier_rep_kernel    : one u64 atomicMin of d^2 << 32 | cell per run of equal rank.
//   frontier_write_kernel  : one thread per slot i < max_frontiers: the record, goal_cells[i] (NONE past the written ones), n_written.
//
// How the workgroups of one launch agree (docs/HISTORY.md, "No cache maintenance inside kernels"): only through relaxed
// device-scope integer atomics whose final value does not depend on order (min, max, add).  No fence, no acquire / release, no
// spinning, no persistent kernel; every loop's bound holds whatever the words hold: a find only follows a strictly smaller parent, a
// unite only goes on with a strictly smaller node.  A load of a parent may be stale: a parent only decreases and every value it held
// is a cell of the same frontier.  What a launch needs of an earlier one comes from the kernel boundary on the stream.
// Checks, sizes, the workspace's layout and the launch geometry are host/frontier_args.h's.
#include "frontier_args.h"
#include "kernels.h"

namespace {
using u64 = unsigned long long;
constexpr int FR_T = FRONTIER_THREADS, FR_TILE = FRONTIER_TILE;
constexpr uint32_t FR_NONE = FRONTIER_NONE;
constexpr u64 FR_NONE64 = ~0ull;

struct FrontierSlot {  // a frontier's running statistics in the workspace
  u64 sum_a, sum_b;
  u64 best;  // cost << 32 | cell, all ones while no member has a cost
  u64 rep;   // d^2 << 32 | cell
  uint32_t min_a, max_a, min_b, max_b;
  uint32_t first_cell, size;
  uint32_t ca, cb;  // the floored centroid
};
static_assert(sizeof(FrontierSlot) == FRONTIER_SLOT_BYTES, "the workspace's layout of host/frontier_args.h");
static_assert(sizeof(svo_grid_frontier) == 48, "the record of include/svo.h");

struct FrontierArgs {
  const uint8_t* cls;
  const uint8_t* blocked;  // or null
  const uint32_t* cost;    // or null
  uint32_t* hdr;           // the workspace: word 0 is n_kept
  FrontierSlot* slots;
  uint32_t* blocks;        // one count, then prefix, per block of FR_T cells
  uint32_t* parent;
  uint32_t* size;
  uint32_t* rank;
  svo_grid_frontier* frontiers;  // the three outputs, null each
  uint32_t* goal_cells;
  uint32_t* label;
  u64* counts;             // or null
  uint32_t n;              // na * nb, at most 2^24
  int na, nb, tb;
  uint32_t free_mask, unknown_mask, min_size, max_frontiers;
  uint32_t seam_cols, seam_cells, scan_blocks;
};

template <int SCOPE>
__device__ __forceinline__ uint32_t fr_load(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, SCOPE); }

// Follows parents while they are strictly smaller: at most x steps whatever the words hold.
template <int SCOPE>
__device__ __forceinline__ uint32_t fr_find(const uint32_t* L, uint32_t x) {
  for (uint32_t p; (p = fr_load<SCOPE>(&L[x])) < x;) x = p;
  return x;
}

// Join the trees of a and b (speckle.hip's uf_unite): each turn hooks the larger of two nodes under the smaller; when the larger was
// no root its former parent has to be joined with b instead, and max(a, b) has strictly decreased.  No waiting.
template <int SCOPE>
__device__ __forceinline__ void fr_unite(uint32_t* L, uint32_t a, uint32_t b) {
  a = fr_find<SCOPE>(L, a);
  b = fr_find<SCOPE>(L, b);
  while (a != b) {
    if (a < b) { const uint32_t t = a; a = b; b = t; }
    const uint32_t old = __hip_atomic_fetch_min(&L[a], b, __ATOMIC_RELAXED, SCOPE);
    if (old >= a) break;  // a was a root (a word never exceeds its index where the tile kernel wrote it)
    a = old;
  }
}

// The exclusive prefix of v over the workgroup and the workgroup's total; sW: FR_T / 64 words of LDS.  Every thread calls it.
__device__ __forceinline__ uint32_t fr_block_scan(uint32_t v, uint32_t* sW, uint32_t& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t x = v;
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t y = __shfl_up(x, o);
    if (lane >= o) x += y;
  }
  if (lane == 63) sW[w] = x;
  __syncthreads();
  uint32_t pre = 0, tot = 0;
  for (int k = 0; k < FR_T / 64; ++k) {
    const uint32_t t = sW[k];
    pre += k < w ? t : 0u;
    tot += t;
  }
  total = tot;
  __syncthreads();  // sW may be written again
  return pre + x - v;
}

// The last lane of this lane's run of equal keys along the wavefront; COMBINE false: every lane is a run of its own.
template <bool COMBINE>
__device__ __forceinline__ int fr_run(uint32_t key, bool& head) {
  const int lane = threadIdx.x & 63;
  if (!COMBINE) { head = true; return lane; }
  const uint32_t before = __shfl_up(key, 1);
  head = lane == 0 || before != key;
  const u64 heads = __ballot(head);
  const u64 later = lane == 63 ? 0ull : heads >> (lane + 1);
  return later ? lane + __ffsll((long long)later) - 1 : 63;
}

struct FrontierSums { uint32_t sa, sb, mna, mxa, mnb, mxb; u64 best; };
}  // namespace

__global__ __launch_bounds__(FR_T) void frontier_tile_kernel(FrontierArgs a) {
  constexpr int P = FR_TILE + 2;
  __shared__ uint8_t sK[P * P];  // bit 0: FREE, bit 1: UNKNOWN; 0 outside the grid
  __shared__ uint32_t sL[FR_T], sC[FR_T];
  __shared__ unsigned sN[3][FR_T / 64];
  const int tid = threadIdx.x;
  const int tia = (int)(blockIdx.x / (unsigned)a.tb), tib = (int)(blockIdx.x - (unsigned)tia * (unsigned)a.tb);
  const int a0 = tia * FR_TILE - 1, b0 = tib * FR_TILE - 1;
  for (int idx = tid; idx < P * P; idx += FR_T) {
    const int ly = idx / P, lx = idx - ly * P;
    const int ga = a0 + ly, gb = b0 + lx;
    const bool in = ga >= 0 && ga < a.na && gb >= 0 && gb < a.nb;
    const size_t cell = in ? (size_t)ga * (size_t)a.nb + (size_t)gb : 0;  // outside the grid: cell 0, read and ignored
    const unsigned c = a.cls[cell];
    const unsigned bl = a.blocked ? a.blocked[cell] : 0u;
    const bool known = in && c < 32u;
    const bool fr = known && ((a.free_mask >> (c & 31u)) & 1u) != 0u && bl == 0u;
    const bool un = known && ((a.unknown_mask >> (c & 31u)) & 1u) != 0u;
    sK[idx] = (uint8_t)((fr ? 1 : 0) | (un ? 2 : 0));
  }
  const int ly = tid / FR_TILE, lx = tid - ly * FR_TILE, li = (ly + 1) * P + lx + 1;
  __syncthreads();
  const unsigned k = sK[li];
  const bool is_free = (k & 1u) != 0u, is_unknown = (k & 2u) != 0u;
  const bool front = is_free && ((sK[li - P] | sK[li + P] | sK[li - 1] | sK[li + 1]) & 2u) != 0u;
  sL[tid] = front ? (uint32_t)tid : FR_NONE;
  sC[tid] = 0u;
  __syncthreads();
  if (front) {  // a word of sL is NONE for good or never: the hooks only lower the others
    constexpr int WG = __HIP_MEMORY_SCOPE_WORKGROUP;
    if (lx > 0 && fr_load<WG>(&sL[tid - 1]) != FR_NONE) fr_unite<WG>(sL, tid, tid - 1);
    if (ly > 0) {
      if (fr_load<WG>(&sL[tid - FR_TILE]) != FR_NONE) fr_unite<WG>(sL, tid, tid - FR_TILE);
      if (lx > 0 && fr_load<WG>(&sL[tid - FR_TILE - 1]) != FR_NONE) fr_unite<WG>(sL, tid, tid - FR_TILE - 1);
      if (lx < FR_TILE - 1 && fr_load<WG>(&sL[tid - FR_TILE + 1]) != FR_NONE) fr_unite<WG>(sL, tid, tid - FR_TILE + 1);
    }
  }
  __syncthreads();
  uint32_t root = FR_NONE;
  if (front) {
    root = fr_find<__HIP_MEMORY_SCOPE_WORKGROUP>(sL, tid);
    __hip_atomic_fetch_add(&sC[root], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  __syncthreads();
  const int ga = a0 + 1 + ly, gb = b0 + 1 + lx;
  if (ga < a.na && gb < a.nb) {
    const size_t cell = (size_t)ga * (size_t)a.nb + (size_t)gb;
    const int ry = (int)root / FR_TILE, rx = (int)root - ry * FR_TILE;
    a.parent[cell] = root == FR_NONE ? FR_NONE : (uint32_t)(a0 + 1 + ry) * (uint32_t)a.nb + (uint32_t)(b0 + 1 + rx);
    a.size[cell] = root == (uint32_t)tid ? sC[tid] : 0u;
  }
  if (!a.counts) return;  // uniform over the launch
  const unsigned n_free = (unsigned)__popcll(__ballot(is_free)), n_unknown = (unsigned)__popcll(__ballot(is_unknown)),
                 n_front = (unsigned)__popcll(__ballot(front));
  if ((tid & 63) == 0) { sN[0][tid >> 6] = n_free; sN[1][tid >> 6] = n_unknown; sN[2][tid >> 6] = n_front; }
  __syncthreads();
  if (tid < 3) {
    unsigned t = 0;
    for (int w = 0; w < FR_T / 64; ++w) t += sN[tid][w];
    if (t) __hip_atomic_fetch_add(&a.counts[tid], (u64)t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// Thread j: first the cells of the columns ib = T, 2T, ..., column by column, then the cells of the rows ia = T, 2T, ..., row by row
// (host/frontier_args.h).  The three neighbours across the seam lie in other tiles, so none of these pairs is united yet.
__global__ __launch_bounds__(FR_T) void frontier_seam_kernel(FrontierArgs a) {
  constexpr int DEV = __HIP_MEMORY_SCOPE_AGENT;
  const uint32_t j = blockIdx.x * FR_T + threadIdx.x;
  if (j >= a.seam_cells) return;
  int ia, ib, ja[3], jb[3];
  if (j < a.seam_cols) {
    const uint32_t s = j / (uint32_t)a.na;
    ia = (int)(j - s * (uint32_t)a.na); ib = (int)(s + 1u) * FR_TILE;
    for (int k = 0; k < 3; ++k) { ja[k] = ia - 1 + k; jb[k] = ib - 1; }
  } else {
    const uint32_t m = j - a.seam_cols, s = m / (uint32_t)a.nb;
    ib = (int)(m - s * (uint32_t)a.nb); ia = (int)(s + 1u) * FR_TILE;
    for (int k = 0; k < 3; ++k) { ja[k] = ia - 1; jb[k] = ib - 1 + k; }
  }
  if (ia >= a.na || ib >= a.nb) return;  // cannot happen with the host's counts
  const uint32_t lq = fr_load<DEV>(&a.parent[(size_t)ia * (size_t)a.nb + (size_t)ib]);
  if (lq == FR_NONE) return;
  for (int k = 0; k < 3; ++k) {
    if (ja[k] < 0 || ja[k] >= a.na || jb[k] < 0 || jb[k] >= a.nb) continue;
    const uint32_t lp = fr_load<DEV>(&a.parent[(size_t)ja[k] * (size_t)a.nb + (size_t)jb[k]]);
    if (lp != FR_NONE && lp < a.n && lq < a.n) fr_unite<DEV>(a.parent, lp, lq);
  }
}

__global__ __launch_bounds__(FR_T) void frontier_size_kernel(FrontierArgs a) {
  const uint32_t p = blockIdx.x * FR_T + threadIdx.x;
  if (p >= a.n) return;
  // nonzero exactly at the tile-local roots.  A root of the grid may see its own word mid-sum: it only tests it against 0, and the
  // word was nonzero before this launch and only grows
  const uint32_t c = a.size[p];
  if (c == 0u) return;
  const uint32_t r = fr_find<__HIP_MEMORY_SCOPE_AGENT>(a.parent, p);
  if (r == p) return;
  __hip_atomic_fetch_add(&a.size[r], c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // nobody adds to size[p]: p is no root
  // The chain of seam hooks is walked once per tile-local root, here, and cut short for everybody after: a min with the root keeps the
  // word a smaller member of the same frontier, so a find that passes through it in this very launch is right either way.
  __hip_atomic_fetch_min(&a.parent[p], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(FR_T) void frontier_count_kernel(FrontierArgs a) {
  __shared__ uint32_t sN[3][FR_T / 64];
  const int tid = threadIdx.x;
  const uint32_t p = blockIdx.x * FR_T + (uint32_t)tid;
  bool root = false, kept = false;
  uint32_t cells = 0;
  if (p < a.n && a.parent[p] == p) {
    const uint32_t s = a.size[p];
    root = true;
    kept = s >= a.min_size;
    cells = kept ? s : 0u;
  }
  for (int o = 32; o > 0; o >>= 1) cells += __shfl_xor(cells, o);
  const uint32_t n_root = (uint32_t)__popcll(__ballot(root)), n_kept = (uint32_t)__popcll(__ballot(kept));
  if ((tid & 63) == 0) { sN[0][tid >> 6] = n_root; sN[1][tid >> 6] = n_kept; sN[2][tid >> 6] = cells; }
  __syncthreads();
  if (tid < 3) {
    uint32_t t = 0;
    for (int w = 0; w < FR_T / 64; ++w) t += sN[tid][w];
    if (tid == 1) a.blocks[blockIdx.x] = t;
    // n_frontiers, n_kept, n_kept_cells: counts[3], [4] and [6]
    if (a.counts && t) __hip_atomic_fetch_add(&a.counts[tid == 2 ? 6 : 3 + tid], (u64)t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__global__ __launch_bounds__(FR_T) void frontier_scan_kernel(FrontierArgs a) {
  __shared__ uint32_t sW[FR_T / 64];
  uint32_t carry = 0;
  for (uint32_t base = 0; base < a.scan_blocks; base += FR_T) {  // the same trip count for every thread
    const uint32_t i = base + threadIdx.x;
    const uint32_t v = i < a.scan_blocks ? a.blocks[i] : 0u;
    uint32_t total;
    const uint32_t pre = fr_block_scan(v, sW, total);
    if (i < a.scan_blocks) a.blocks[i] = carry + pre;
    carry += total;
  }
  if (threadIdx.x == 0) a.hdr[0] = carry;
}

__global__ __launch_bounds__(FR_T) void frontier_rank_kernel(FrontierArgs a) {
  __shared__ uint32_t sW[FR_T / 64];
  const uint32_t p = blockIdx.x * FR_T + threadIdx.x;
  uint32_t s = 0;
  const bool kept = p < a.n && a.parent[p] == p && (s = a.size[p]) >= a.min_size;
  uint32_t total;
  const uint32_t rk = a.blocks[blockIdx.x] + fr_block_scan(kept ? 1u : 0u, sW, total);
  if (p >= a.n) return;
  a.rank[p] = kept ? rk : FR_NONE;
  if (kept && rk < a.max_frontiers) {
    FrontierSlot z;
    z.sum_a = z.sum_b = 0; z.best = z.rep = FR_NONE64;
    z.min_a = z.min_b = FR_NONE; z.max_a = z.max_b = 0u;
    z.first_cell = p; z.size = s; z.ca = z.cb = 0u;
    a.slots[rk] = z;
  }
}

template <bool COMBINE>
__global__ __launch_bounds__(FR_T) void frontier_stats_kernel(FrontierArgs a) {
  const int lane = threadIdx.x & 63;
  const uint32_t p = blockIdx.x * FR_T + threadIdx.x;
  uint32_t rk = FR_NONE;
  if (p < a.n) {
    const uint32_t l = a.parent[p];
    if (l != FR_NONE) {
      const uint32_t r = fr_find<__HIP_MEMORY_SCOPE_AGENT>(a.parent, p);
      rk = a.rank[r];                // NONE where the frontier is not kept
      if (r != p) a.rank[p] = rk;    // per cell from here on; nobody reads the rank of a cell that is no root in this launch
    }
    if (a.label) a.label[p] = rk;
  }
  const uint32_t key = rk < a.max_frontiers ? rk : FR_NONE;
  const uint32_t ia = p < a.n ? p / (uint32_t)a.nb : 0u, ib = p < a.n ? p - ia * (uint32_t)a.nb : 0u;
  FrontierSums v;
  v.sa = v.mna = v.mxa = ia;
  v.sb = v.mnb = v.mxb = ib;
  v.best = FR_NONE64;
  if (key != FR_NONE && a.cost) {
    const uint32_t c = a.cost[p];
    if (c != FR_NONE) v.best = (u64)c << 32 | (u64)p;
  }
  bool head;
  const int end = fr_run<COMBINE>(key, head);
  if (COMBINE) {
    for (int o = 1; o < 64; o <<= 1) {  // lane i holds its run's cells i .. min(i + 2o - 1, end) afterwards
      FrontierSums w;
      w.sa = __shfl_down(v.sa, o); w.sb = __shfl_down(v.sb, o);
      w.mna = __shfl_down(v.mna, o); w.mxa = __shfl_down(v.mxa, o);
      w.mnb = __shfl_down(v.mnb, o); w.mxb = __shfl_down(v.mxb, o);
      w.best = __shfl_down(v.best, o);
      if (lane + o <= end) {
        v.sa += w.sa; v.sb += w.sb;  // at most 64 * 8191 each
        v.mna = min(v.mna, w.mna); v.mxa = max(v.mxa, w.mxa);
        v.mnb = min(v.mnb, w.mnb); v.mxb = max(v.mxb, w.mxb);
        v.best = min(v.best, w.best);
      }
    }
  }
  if (!head || key == FR_NONE) return;
  constexpr int DEV = __HIP_MEMORY_SCOPE_AGENT;
  FrontierSlot* const s = &a.slots[key];
  __hip_atomic_fetch_add(&s->sum_a, (u64)v.sa, __ATOMIC_RELAXED, DEV);
  __hip_atomic_fetch_add(&s->sum_b, (u64)v.sb, __ATOMIC_RELAXED, DEV);
  __hip_atomic_fetch_min(&s->min_a, v.mna, __ATOMIC_RELAXED, DEV);
  __hip_atomic_fetch_max(&s->max_a, v.mxa, __ATOMIC_RELAXED, DEV);
  __hip_atomic_fetch_min(&s->min_b, v.mnb, __ATOMIC_RELAXED, DEV);
  __hip_atomic_fetch_max(&s->max_b, v.mxb, __ATOMIC_RELAXED, DEV);
  if (v.best != FR_NONE64) __hip_atomic_fetch_min(&s->best, v.best, __ATOMIC_RELAXED, DEV);
}

__global__ __launch_bounds__(FR_T) void frontier_centroid_kernel(FrontierArgs a) {
  const uint32_t i = blockIdx.x * FR_T + threadIdx.x;
  if (i >= min(a.hdr[0], a.max_frontiers)) return;
  FrontierSlot* const s = &a.slots[i];
  const u64 size = s->size ? s->size : 1u;  // a kept frontier has min_size >= 1 cells
  s->ca = (uint32_t)(s->sum_a / size);
  s->cb = (uint32_t)(s->sum_b / size);
}

template <bool COMBINE>
__global__ __launch_bounds__(FR_T) void frontier_rep_kernel(FrontierArgs a) {
  const int lane = threadIdx.x & 63;
  const uint32_t p = blockIdx.x * FR_T + threadIdx.x;
  const uint32_t rk = p < a.n ? a.rank[p] : FR_NONE;
  const uint32_t key = rk < a.max_frontiers ? rk : FR_NONE;
  u64 v = FR_NONE64;
  if (key != FR_NONE) {
    const int ia = (int)(p / (uint32_t)a.nb), ib = (int)(p - (uint32_t)ia * (uint32_t)a.nb);
    const int da = ia - (int)a.slots[key].ca, db = ib - (int)a.slots[key].cb;
    v = (u64)(uint32_t)(da * da + db * db) << 32 | (u64)p;  // d^2 < 2^27
  }
  bool head;
  const int end = fr_run<COMBINE>(key, head);
  if (COMBINE) {
    for (int o = 1; o < 64; o <<= 1) {
      const u64 w = __shfl_down(v, o);
      if (lane + o <= end) v = min(v, w);
    }
  }
  if (head && key != FR_NONE) __hip_atomic_fetch_min(&a.slots[key].rep, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(FR_T) void frontier_write_kernel(FrontierArgs a) {
  const uint32_t i = blockIdx.x * FR_T + threadIdx.x;
  if (i >= a.max_frontiers) return;
  const uint32_t n_written = min(a.hdr[0], a.max_frontiers);
  if (i == 0 && a.counts && n_written) __hip_atomic_fetch_add(&a.counts[5], (u64)n_written, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (i >= n_written) {
    if (a.goal_cells) a.goal_cells[i] = FR_NONE;
    return;
  }
  const FrontierSlot s = a.slots[i];
  const uint32_t rep = (uint32_t)(s.rep & 0xFFFFFFFFull);
  if (a.goal_cells) a.goal_cells[i] = rep;
  if (a.frontiers) {
    svo_grid_frontier f;
    f.first_cell = s.first_cell; f.size = s.size; f.rep_cell = rep;
    f.best_cell = (uint32_t)(s.best & 0xFFFFFFFFull); f.best_cost = (uint32_t)(s.best >> 32);  // both NONE while no member has a cost
    f.min_a = (uint16_t)s.min_a; f.max_a = (uint16_t)s.max_a; f.min_b = (uint16_t)s.min_b; f.max_b = (uint16_t)s.max_b;
    f.reserved = 0u;
    f.sum_a = s.sum_a; f.sum_b = s.sum_b;
    a.frontiers[i] = f;
  }
}

// ----------------------------------------------------------------------------- host side
extern "C" int svo_grid_frontier_default_params(const svo_grid_clearance_params* clearance, svo_grid_frontier_params* out) {
  return frontier_default_params(clearance, out);
}

extern "C" size_t svo_grid_frontier_workspace_bytes(int na, int nb, int max_frontiers) { return frontier_workspace_bytes(na, nb, max_frontiers); }

extern "C" int svo_grid_frontier_set_mode(svo_ctx* ctx, int combine) {
  if (!ctx) return SVO_ERR_INVALID;
  ctx->frontier_combine = combine ? 1 : 0;
  return SVO_OK;
}

extern "C" int svo_grid_frontiers_dev(svo_ctx* ctx, const uint8_t* cls, const uint8_t* blocked, const uint32_t* cost,
                                      const svo_grid_frontier_params* prm, void* workspace, const svo_grid_frontier_out* out,
                                      uint64_t* counts) {
  if (!ctx) return SVO_ERR_INVALID;
  svo_use_device(ctx);
  SVO_ARGS_CHECK(ctx, frontier_check(cls, cost, prm, workspace, out, counts, true, &err));
  const int na = prm->na, nb = prm->nb, mf = prm->max_frontiers;
  unsigned char* const ws = static_cast<unsigned char*>(workspace);
  FrontierArgs a{};
  a.cls = cls; a.blocked = blocked; a.cost = cost;
  a.hdr = reinterpret_cast<uint32_t*>(ws);
  a.slots = reinterpret_cast<FrontierSlot*>(ws + frontier_ws_slots_offset());
  a.blocks = reinterpret_cast<uint32_t*>(ws + frontier_ws_blocks_offset(mf));
  a.parent = reinterpret_cast<uint32_t*>(ws + frontier_ws_cells_offset(0, na, nb, mf));
  a.size = reinterpret_cast<uint32_t*>(ws + frontier_ws_cells_offset(1, na, nb, mf));
  a.rank = reinterpret_cast<uint32_t*>(ws + frontier_ws_cells_offset(2, na, nb, mf));
  a.frontiers = out->frontiers; a.goal_cells = out->goal_cells; a.label = out->label;
  a.counts = reinterpret_cast<u64*>(counts);
  a.n = (uint32_t)na * (uint32_t)nb; a.na = na; a.nb = nb; a.tb = (int)frontier_tiles_along(nb);
  a.free_mask = prm->free_mask; a.unknown_mask = prm->unknown_mask; a.min_size = prm->min_size; a.max_frontiers = (uint32_t)mf;
  a.seam_cols = (uint32_t)frontier_seam_cols(na, nb); a.seam_cells = (uint32_t)frontier_seam_cells(na, nb);
  a.scan_blocks = (uint32_t)frontier_scan_blocks(na, nb);
  const dim3 cells((unsigned)a.scan_blocks), wg(FR_T), slots((unsigned)frontier_groups((size_t)mf));
  const bool combine = ctx->frontier_combine != 0;
  hipStream_t st = ctx->stream;
  SvoProfScope prof(ctx, SVO_PROF_GRID_FRONTIER);
  if (counts) SVO_HIP_CHECK(ctx, hipMemsetAsync(counts, 0, 8 * sizeof(u64), st));
  hipLaunchKernelGGL(frontier_tile_kernel, dim3((unsigned)frontier_tiles(na, nb)), wg, 0, st, a);
  if (a.seam_cells) hipLaunchKernelGGL(frontier_seam_kernel, dim3((unsigned)frontier_groups(a.seam_cells)), wg, 0, st, a);
  hipLaunchKernelGGL(frontier_size_kernel, cells, wg, 0, st, a);
  hipLaunchKernelGGL(frontier_count_kernel, cells, wg, 0, st, a);
  hipLaunchKernelGGL(frontier_scan_kernel, dim3(1), wg, 0, st, a);
  hipLaunchKernelGGL(frontier_rank_kernel, cells, wg, 0, st, a);
  if (combine) hipLaunchKernelGGL(frontier_stats_kernel<true>, cells, wg, 0, st, a);
  else hipLaunchKernelGGL(frontier_stats_kernel<false>, cells, wg, 0, st, a);
  hipLaunchKernelGGL(frontier_centroid_kernel, slots, wg, 0, st, a);
  if (combine) hipLaunchKernelGGL(frontier_rep_kernel<true>, cells, wg, 0, st, a);
  else hipLaunchKernelGGL(frontier_rep_kernel<false>, cells, wg, 0, st, a);
  hipLaunchKernelGGL(frontier_write_kernel, slots, wg, 0, st, a);
  SVO_HIP_CHECK(ctx, hipGetLastError());
  return SVO_OK;
}

extern "C" int svo_grid_frontiers(svo_ctx* ctx, const uint8_t* cls, const uint8_t* blocked, const uint32_t* cost,
                                  const svo_grid_frontier_params* prm, const svo_grid_frontier_out* out, uint64_t* counts) {
  if (!ctx) return SVO_ERR_INVALID;
  svo_use_device(ctx);
  SVO_ARGS_CHECK(ctx, frontier_check(cls, cost, prm, nullptr, out, counts, false, &err));
  const size_t n = (size_t)prm->na * (size_t)prm->nb, mf = (size_t)prm->max_frontiers, b_rec = mf * sizeof(svo_grid_frontier);
  SvoParts parts;
  const size_t o_counts = parts.add(8 * sizeof(u64)), o_ws = parts.add(frontier_workspace_bytes(prm->na, prm->nb, prm->max_frontiers)),
               o_rec = parts.add(b_rec), o_cost = parts.add(4 * n), o_label = parts.add(4 * n), o_goal = parts.add(4 * mf), o_cls = parts.add(n),
               o_blocked = parts.add(n);
  SvoTemp d;
  SVO_HIP_CHECK(ctx, hipMalloc(&d.p, parts.total()));
  svo_grid_frontier_out o{};
  o.frontiers = out->frontiers ? d.at<svo_grid_frontier>(o_rec) : nullptr;  // what the caller did not ask for is not written
  o.goal_cells = out->goal_cells ? d.at<uint32_t>(o_goal) : nullptr;
  o.label = out->label ? d.at<uint32_t>(o_label) : nullptr;
  u64 c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  hipStream_t st = ctx->stream;
  // The caller's frontiers go up first, so that the records the contract leaves untouched come back as they were.
  hipError_t e = hipMemcpyAsync(d.at(o_cls), cls, n, hipMemcpyHostToDevice, st);
  if (e == hipSuccess && blocked) e = hipMemcpyAsync(d.at(o_blocked), blocked, n, hipMemcpyHostToDevice, st);
  if (e == hipSuccess && cost) e = hipMemcpyAsync(d.at(o_cost), cost, 4 * n, hipMemcpyHostToDevice, st);
  if (e == hipSuccess && out->frontiers) e = hipMemcpyAsync(o.frontiers, out->frontiers, b_rec, hipMemcpyHostToDevice, st);
  const int rc = svo_host_call(
      ctx, "grid_frontier", e,
      [&] {
        return svo_grid_frontiers_dev(ctx, d.at(o_cls), blocked ? d.at(o_blocked) : nullptr, cost ? d.at<uint32_t>(o_cost) : nullptr, prm, d.at(o_ws),
                                      &o, d.at<uint64_t>(o_counts));
      },
      [&] {
        hipError_t e = hipSuccess;
        if (out->frontiers) e = hipMemcpyAsync(out->frontiers, o.frontiers, b_rec, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && out->goal_cells) e = hipMemcpyAsync(out->goal_cells, o.goal_cells, 4 * mf, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && out->label) e = hipMemcpyAsync(out->label, o.label, 4 * n, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(c, d.at(o_counts), sizeof(c), hipMemcpyDeviceToHost, st);
        return e;
      });
  if (rc) return rc;
  if (counts) for (int k = 0; k < 8; ++k) counts[k] = c[k];
  return SVO_OK;
}
