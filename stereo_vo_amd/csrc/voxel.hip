// Voxel map (include/svo.h, "voxel map"): a sparse voxel grid in HBM, an open-addressing hash table into which clouds of
// svo_cloud_point records are fused under a camera->world transform, and from which the occupied voxels come back as a point list.
//
//   voxel_insert_kernel  : one thread per record, 256-thread workgroups.  Key and payload per record in f64 / integers exactly as
//                          the header states.  Clouds are in raster order, so neighbouring lanes very often fall into one voxel and
//                          same-address atomics would serialise: the runs of equal keys inside a wavefront are summed into their
//                          first lane (a segmented sum, see below) and only those run heads probe (64-bit atomicCAS on keys[],
//                          linear, at most SVO_VOXEL_MAX_PROBES slots) and issue the four atomicAdds.  Integer sums commute, so the
//                          table is the same with or without the merge.  The four counters get one atomicAdd per workgroup each.
//   voxel_remove_kernel  : the insert's exact inverse: the insert's front half and wavefront merge, then a run head
//                          FINDS its slot by plain loads (it never claims: keys[] and the map's counters are only read)
//                          and subtracts its sums, saturating at 0 per field: one 64-bit CAS loop on the count | intensity word,
//                          then either three saturating CAS loops on the sums or, in the step that takes the count to 0, three
//                          non-returning atomic ANDs with 0.  No thread can see a wrapped word, so the result depends on no order.
//   voxel_extract_kernel : VX_ITEMS * 256 slots per workgroup; svo_compact_slot inside the workgroup, one returning atomicAdd per
//                          workgroup for its base in the output (whose order is free), one for its share of n_stored.
//
//   voxel_carve_kernel   : the extraction's tiling, one thread per slot (keys first, payload only where live).  A live voxel's mean
//                          is projected into a keyframe's disparity map in f64 as the header states, the window around the pixel
//                          is read, and a voxel the keyframe saw through gets its four payload words zeroed by plain stores: its
//                          own slot, which no other thread of the launch touches.  The key stays, so no probe chain changes.
//                          Slots sit where the hash put them, so the lanes of a wavefront read unrelated pixels: a gather that
//                          no ordering of the table's walk would coalesce.  A keyframe map (0.9 MB at 1241 x 376) stays in L2; each window
//                          row is 2 radius + 1 adjacent shorts, read by a wavefront-uniform loop (no lane-dependent trip count).
//   voxel_copy_kernel    : the same tiling over src; a qualifying slot probes dst by vx_probe, the insert's loop, and adds its
//                          four words with the insert's four atomicAdds.
//
//   voxel_splat_kernel   : the map seen from a pose.  The carve's tiling and its projection; a qualifying voxel in front
//                          of the camera becomes a (2 r + 1)^2 footprint of one 32-bit value, disparity << 8 | mean intensity, and
//                          every pixel of it takes the maximum by a relaxed atomicMax on the caller's workspace.  The trip count
//                          of a footprint depends on the lane (1 .. 33^2 pixels), so footprints with r > 1 are collected by a
//                          ballot and drawn by the whole wavefront in turn, 64 pixels of consecutive columns per step; the small
//                          ones are drawn by their own lane (1.7 to 3.8 times faster than every lane drawing its own).
//                          Optionally a plain load skips the atomic where the pixel already holds at least the value: values only
//                          grow within the launch and the memset precedes it on the stream, so a stale load costs a needless
//                          atomic, never a wrong skip.  It is OFF by default: the wait for the load costs more than the atomics
//                          it saves on three of the four measured maps.  Neither choice can change the image.
//   voxel_resolve_kernel : the workspace -> the CV_16S map and the u8 image, four pixels per thread (16-byte load, 8-byte and 4-byte
//                          stores where the pointers allow it, else and in the tail pixel by pixel); counts the covered pixels.
//
//   voxel_grid_kernel    : the ground plan.  The carve's tiling; keys first, ci where occupied, the up axis's sum word
//                          where the slot qualifies (24 B per qualifying slot), integers and f32 only: a qualifying voxel inside the
//                          height band is binned by its key into a cell of the caller's workspace by two 64-bit atomic max and two
//                          64-bit atomic adds whose values are not read back.  The lanes of a wavefront address unrelated cells;
//                          nothing is merged inside the wavefront (no such form was built).  Optionally a relaxed load skips a max
//                          atomic where the word already holds at least the value (svo_voxel_grid_set_mode; DESIGN §7j has the
//                          figures and the default); it cannot change a bit.
//   voxel_grid_resolve_kernel : the cells -> class, top, bottom, intensity and the two tallies, one cell per thread; counts the
//                          occupied cells and the obstacles.
//
// Nothing passes between workgroups except order-independent relaxed device-scope atomics (docs/HISTORY.md, "No cache maintenance
// inside kernels"): no fence, no acquire / release, no waiting.  In a launch that CLAIMS slots (insert, copy) the CAS's RETURN value
// decides a probe, never a plain load; a launch that claims nothing (extraction, carve, splat, removal) reads keys an earlier launch
// on the same stream wrote, and there a load may decide.  The payload words are added to by inserts and copies, subtracted from
// (saturating) by a removal, zeroed by a carve (a launch of its own, ordered by the stream, each thread its own slot), and are read
// by a LATER launch on the same stream (extraction, carve, copy, download).  A full table costs at most 64 probes per run head:
// bounded work, no spinning; the removal's CAS loops retry only when another head's subtraction got in first, and every head
// subtracts a bounded number of times.
//
// Written once: vx_record, vx_merge (insert, removal), vx_probe, vx_add (insert, copy), vx_walk_first (the table walks), vx_mean
// (extraction, carve, splat), vx_to_camera, vx_pixel (carve, splat), vx_wave_sum, vx_tally (every count but the copy's).  The host
// logic that needs no GPU (argument checks, pose7 -> matrix, the box, launch geometry) is host/voxel_args.h.
#include "kernels.h"
#include "tail_device.h"
#include "voxel_args.h"
#include "voxel_ledger.h"

namespace {
typedef unsigned long long u64;
constexpr int VX_T = VOXEL_THREADS;
constexpr int VX_ITEMS = VOXEL_WALK_ITEMS;  // slots per thread of a launch that walks the table
constexpr u64 VX_EMPTY = ~0ull;
constexpr double VX_LIMIT = 1048576.0;  // 2^20 voxels either side of the origin per axis

struct VoxelTable {
  u64 *keys, *ci, *sx, *sy, *sz;  // cap each (the download's layout, in this order)
  u64* counters;                  // n_voxels, n_inserted, n_rejected, n_dropped
  u64 mask;                       // cap - 1
};

struct VoxelInsertArgs {
  const svo_cloud_point* pts;
  int n;
  double m[12];
  float voxel_size, max_depth;
  VoxelTable t;
};

struct VoxelRemoveArgs : VoxelInsertArgs {
  u64* counts;  // {n_removed, n_rejected, n_missing, n_short}, zeroed on the stream before the launch; or null
};

struct VoxelExtractArgs {
  VoxelTable t;
  unsigned min_count;
  float voxel_size;
  svo_cloud_point* out;
  int max_points;
  int* counts;  // {n_total, n_stored}, zeroed on the stream before the launch
};

__host__ __device__ __forceinline__ u64 vx_fmix64(u64 k) {
  k ^= k >> 33; k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return k;
}

// The probe loop of the contract, written once: linear from the home slot, at most SVO_VOXEL_MAX_PROBES 64-bit CASes of keys[h]
// from EMPTY to key, whose RETURN value decides.  0: no slot (dropped), 1: found, 2: claimed; h is the slot for 1 and 2.
__device__ __forceinline__ int vx_probe(const VoxelTable& t, u64 key, u64& h) {
  h = vx_fmix64(key) & t.mask;
  for (int p = 0; p < SVO_VOXEL_MAX_PROBES; ++p) {
    u64 expected = VX_EMPTY;
    __hip_atomic_compare_exchange_strong(&t.keys[h], &expected, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (expected == VX_EMPTY) return 2;
    if (expected == key) return 1;
    h = (h + 1) & t.mask;
  }
  return 0;
}

__device__ __forceinline__ void vx_add(const VoxelTable& t, u64 h, u64 ci, u64 sx, u64 sy, u64 sz) {
  __hip_atomic_fetch_add(&t.ci[h], ci, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_fetch_add(&t.sx[h], sx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_fetch_add(&t.sy[h], sy, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_fetch_add(&t.sz[h], sz, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct VoxelCarveArgs {
  VoxelTable t;
  const int16_t* disp;
  int width, height, radius, margin16;
  unsigned keep_count;
  float voxel_size;
  double m[12];
  double focal, cx, cy, baseline;
  u64* counts;  // {n_live, n_tested, n_carved}, zeroed on the stream before the launch; or null
};

struct VoxelCopyArgs {
  VoxelTable src, dst;
  unsigned min_count;
  int boxed;
  int klo[3], khi[3];
};

struct VoxelSplatArgs {
  VoxelTable t;
  unsigned* pix;  // width * height, zeroed on the stream before the launch
  int width, height, max_radius;
  unsigned min_count;
  float voxel_size;
  double m[12];
  double focal, cx, cy, baseline;
  u64* counts;  // {n_qualifying, n_drawn, n_splat, n_pixels}, zeroed on the stream before the launch; or null
};

struct VoxelResolveArgs {
  const unsigned* pix;
  int16_t* disp;
  uint8_t* inten;  // or null
  size_t n;        // width * height
  int vec;         // pix 16-byte, disp 8-byte and inten 4-byte aligned: the vector form
  u64* counts;
};

struct VoxelGridArgs {
  const u64 *keys, *ci, *sup;  // sup: the up axis's sum words, chosen by the host among sx / sy / sz
  size_t cap;
  u64* cells;  // 4 words per cell {top, bot, nvox, npts}, zeroed on the stream before the launch
  int shift_up, shift_a, shift_b;  // 21 * axis: where each axis's index sits in a key
  int up_sign, ka0, kb0, cell_voxels, na, nb;
  unsigned min_count;
  long long hlo, hhi;
  u64* counts;  // {n_qualifying, n_in_band, n_binned, n_cells, n_obstacle}, zeroed on the stream before the launch; or null
};

struct VoxelGridResolveArgs {
  const u64* cells;
  size_t n;  // na * nb
  long long step;
  float voxel_size;
  svo_voxel_grid_out o;
  u64* counts;
};
}  // namespace

struct svo_voxel_map {
  svo_ctx* ctx = nullptr;
  svo_voxel_map_params prm{};
  size_t cap = 0;
  u64* d_mem = nullptr;  // keys | ci | sx | sy | sz | 4 counters | 2 ints of the synchronous extraction
  VoxelTable t{};
  int* d_counts = nullptr;
  int render_coop = 1, render_pre = 0;  // svo_voxel_render_set_mode; the defaults are the measured choice
  int grid_pre = 0;                     // svo_voxel_grid_set_mode; likewise
};

// The counts of a launch.  vx_wave_sum: per-thread tallies -> their sums over the wavefront, in every lane.  vx_tally: a wavefront's
// totals -> LDS -> one atomicAdd per non-zero total of the workgroup, total k to dst[k].
template <int N, typename T>
__device__ __forceinline__ void vx_wave_sum(T (&n)[N]) {
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int k = 0; k < N; ++k) n[k] += __shfl_xor(n[k], o);
  }
}
template <int N, typename T>
__device__ __forceinline__ void vx_tally(const T (&n)[N], u64* dst) {
  __shared__ T sC[N][VX_T / 64];
  const int tid = threadIdx.x;
  if ((tid & 63) == 0) {
#pragma unroll
    for (int k = 0; k < N; ++k) sC[k][tid >> 6] = n[k];
  }
  __syncthreads();
  if (tid < N) {
    T t = 0;
    for (int w = 0; w < VX_T / 64; ++w) t += sC[tid][w];
    if (t) __hip_atomic_fetch_add(&dst[tid], (u64)t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// The front half of the insert and of the removal (items 1-3 of the contract: reject, transform, key and fractions).  A rejected (or
// absent) record leaves key = EMPTY and a zero contribution.
__device__ __forceinline__ void vx_record(const VoxelInsertArgs& a, size_t i, bool valid, u64& key, unsigned& ci, unsigned& fx, unsigned& fy, unsigned& fz) {
  key = VX_EMPTY;
  ci = 0; fx = 0; fy = 0; fz = 0;  // ci of one record: count << 16 | intensity (a run of 64 sums to < 2^23 | 2^14)
  if (valid) {
    const svo_cloud_point p = a.pts[i];  // one 16-byte load (global memory takes it at 4-byte alignment)
    const float x = p.x, y = p.y, z = p.z;
    const unsigned tag = p.tag;
    if (z > 0.0f && !(a.max_depth > 0.0f && z > a.max_depth)) {
      const double xd = (double)x, yd = (double)y, zd = (double)z, vs = (double)a.voxel_size;
      double q[3];
      bool in = true;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const double w = a.m[4 * r] * xd + a.m[4 * r + 1] * yd + a.m[4 * r + 2] * zd + a.m[4 * r + 3];
        q[r] = w / vs;
        in = in && q[r] >= -VX_LIMIT && q[r] < VX_LIMIT;
      }
      if (in) {
        u64 k[3];
        unsigned f[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          const double fl = floor(q[r]);
          k[r] = (u64)((long long)fl + (1ll << 20));
          const u64 fr = (u64)floor((q[r] - fl) * 65536.0);
          f[r] = (unsigned)(fr < 65535ull ? fr : 65535ull);
        }
        key = k[0] | (k[1] << 21) | (k[2] << 42);
        ci = (1u << 16) | (tag >> 24);
        fx = f[0]; fy = f[1]; fz = f[2];
      }
    }
  }
}

// The wavefront merge: the runs of equal keys inside a wavefront are summed into their first lane.  Returns whether
// this lane is a run head; afterwards a head holds its run's sums.
__device__ __forceinline__ bool vx_merge(int lane, u64 key, unsigned& ci, unsigned& fx, unsigned& fy, unsigned& fz) {
  // run heads: lane 0, or a key other than the lane before's (rejected records carry EMPTY: they form runs too and never probe)
  const u64 prev = __shfl_up(key, 1);
  const bool head = lane == 0 || prev != key;
  const u64 heads = __ballot(head);
  // segmented sum: after the round with offset o a lane holds the sum over [lane, min(lane + 2 o, end of its run)); the rounds
  // stop (wavefront-uniformly) once no lane has a partner inside its run, which is at once when nothing merges
  const u64 after = lane == 63 ? 0ull : heads >> (lane + 1);
  const int end = after ? lane + 1 + __builtin_ctzll(after) : 64;
  for (int o = 1; o < 64; o <<= 1) {
    const bool take = lane + o < end;
    if (!__ballot(take)) break;
    const unsigned c = __shfl_down(ci, o), sx = __shfl_down(fx, o), sy = __shfl_down(fy, o), sz = __shfl_down(fz, o);
    if (take) { ci += c; fx += sx; fy += sy; fz += sz; }
  }
  return head;
}

__global__ __launch_bounds__(VX_T) void voxel_insert_kernel(VoxelInsertArgs a) {
  const int tid = threadIdx.x, lane = tid & 63;
  const size_t i = (size_t)blockIdx.x * VX_T + (size_t)tid;
  const bool valid = i < (size_t)a.n;
  u64 key;
  unsigned ci, fx, fy, fz;
  vx_record(a, i, valid, key, ci, fx, fy, fz);
  const bool head = vx_merge(lane, key, ci, fx, fy, fz);
  bool claimed = false, dropped = false;
  if (head && key != VX_EMPTY) {
    u64 h;
    const int got = vx_probe(a.t, key, h);
    claimed = got == 2;
    if (got) vx_add(a.t, h, ((u64)(ci >> 16) << 40) | (u64)(ci & 0xFFFFu), (u64)fx, (u64)fy, (u64)fz);
    else dropped = true;
  }
  // counters, in points: ballots only, except for the dropped points, which exist only once the table overflows
  const unsigned n_valid = (unsigned)__popcll(__ballot(valid));
  const unsigned n_rej = (unsigned)__popcll(__ballot(valid && key == VX_EMPTY));
  const unsigned n_claim = (unsigned)__popcll(__ballot(claimed));
  unsigned n_drop = 0;
  if (__ballot(dropped)) {
    n_drop = dropped ? ci >> 16 : 0u;
    for (int o = 32; o > 0; o >>= 1) n_drop += __shfl_xor(n_drop, o);
  }
  const unsigned n[4] = {n_claim, n_valid - n_rej - n_drop, n_rej, n_drop};
  vx_tally(n, a.t.counters);
}

// The removal's find (item 2 of "Voxel map removal"): the insert's walk with a load in place of the CAS.  A removal writes no key, and
// every key it reads was written by an earlier launch on the same stream, so here a load may decide.
__device__ __forceinline__ bool vx_find(const VoxelTable& t, u64 key, u64& h) {
  h = vx_fmix64(key) & t.mask;
  for (int p = 0; p < SVO_VOXEL_MAX_PROBES; ++p) {
    const u64 k = t.keys[h];
    if (k == key) return true;
    if (k == VX_EMPTY) return false;
    h = (h + 1) & t.mask;
  }
  return false;
}

// *p = max(0, *p - v): a compare-and-swap loop whose every step is the saturating subtraction of the value it replaces, so that no
// other thread ever sees a wrapped word.
__device__ __forceinline__ void vx_sub_sat(u64* p, u64 v) {
  if (v == 0ull) return;
  u64 old = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  while (old != 0ull) {
    const u64 now = old > v ? old - v : 0ull;
    if (__hip_atomic_compare_exchange_strong(p, &old, now, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
  }
}

__global__ __launch_bounds__(VX_T) void voxel_remove_kernel(VoxelRemoveArgs a) {
  const int tid = threadIdx.x, lane = tid & 63;
  const size_t i = (size_t)blockIdx.x * VX_T + (size_t)tid;
  const bool valid = i < (size_t)a.n;
  u64 key;
  unsigned ci, fx, fy, fz;
  vx_record(a, i, valid, key, ci, fx, fy, fz);
  const bool head = vx_merge(lane, key, ci, fx, fy, fz);
  bool missing = false;
  unsigned n_short = 0;
  if (head && key != VX_EMPTY) {
    u64 h;
    if (vx_find(a.t, key, h)) {
      // count and intensity sum share a word: one CAS applies item 3 to both.  Once the count is 0 the word is 0 and stays 0.
      const u64 C = (u64)(ci >> 16), I = (u64)(ci & 0xFFFFu), lo40 = (1ull << 40) - 1ull;
      u64 old = __hip_atomic_load(&a.t.ci[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), count, left;
      for (;;) {
        count = old >> 40;
        left = count > C ? count - C : 0ull;
        const u64 isum = old & lo40;
        const u64 now = left ? (left << 40) | (isum > I ? isum - I : 0ull) : 0ull;
        if (now == old) break;
        if (__hip_atomic_compare_exchange_strong(&a.t.ci[h], &old, now, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
      }
      n_short = (unsigned)(C - (count - left));
      if (left) {
        vx_sub_sat(&a.t.sx[h], (u64)fx); vx_sub_sat(&a.t.sy[h], (u64)fy); vx_sub_sat(&a.t.sz[h], (u64)fz);
      } else if (count) {  // the step that emptied the voxel: whatever the other heads still subtract, 0 stays 0
        __hip_atomic_fetch_and(&a.t.sx[h], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_and(&a.t.sy[h], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_and(&a.t.sz[h], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    } else {
      missing = true;
    }
  }
  if (!a.counts) return;  // uniform over the launch
  // counts, in points: ballots, and sums only where a wavefront has something to sum
  const unsigned n_valid = (unsigned)__popcll(__ballot(valid));
  const unsigned n_rej = (unsigned)__popcll(__ballot(valid && key == VX_EMPTY));
  unsigned n_miss = 0;
  if (__ballot(missing)) {
    n_miss = missing ? ci >> 16 : 0u;
    for (int o = 32; o > 0; o >>= 1) n_miss += __shfl_xor(n_miss, o);
  }
  if (__ballot(n_short != 0u)) {
    for (int o = 32; o > 0; o >>= 1) n_short += __shfl_xor(n_short, o);
  }
  const unsigned n[4] = {n_valid - n_rej - n_miss, n_rej, n_miss, n_short};
  vx_tally(n, a.counts);
}

// The first slot of this thread in a launch that walks the table: VX_ITEMS slots per thread, VX_T apart.
__device__ __forceinline__ size_t vx_walk_first() { return (size_t)blockIdx.x * (VX_T * VX_ITEMS) + (size_t)threadIdx.x; }

// Axis r of a voxel's mean point in map units: its key's index plus the mean fraction, times the voxel size.
__device__ __forceinline__ double vx_mean(u64 key, int r, u64 sum, u64 count, double vs) {
  const double k = (double)((long long)((key >> (21 * r)) & 0x1FFFFFull) - (1ll << 20));
  return (k + (double)sum / ((double)count * 65536.0)) * vs;
}

// q = [R | t] p with the launch's 3 x 4 world->camera matrix, and a pixel coordinate of q rounded to the nearest (as a double:
// the caller's range test is what NaN and infinity fail).
template <typename Args>
__device__ __forceinline__ double vx_to_camera(const Args& a, int r, const double (&p)[3]) {
  return a.m[4 * r] * p[0] + a.m[4 * r + 1] * p[1] + a.m[4 * r + 2] * p[2] + a.m[4 * r + 3];
}
__device__ __forceinline__ double vx_pixel(double focal, double q, double qz, double centre) { return floor(focal * q / qz + centre + 0.5); }

__global__ __launch_bounds__(VX_T) void voxel_extract_kernel(VoxelExtractArgs a) {
  __shared__ int sW[VX_T / 64];
  __shared__ int sBase;
  const size_t cap = (size_t)a.t.mask + 1;
  const size_t first = vx_walk_first();
  int slot[VX_ITEMS];
  u64 ci[VX_ITEMS];
  int total = 0;
#pragma unroll
  for (int j = 0; j < VX_ITEMS; ++j) {
    const size_t s = first + (size_t)j * VX_T;
    bool keep = false;
    ci[j] = 0;
    if (s < cap && a.t.keys[s] != VX_EMPTY) {
      ci[j] = a.t.ci[s];
      keep = (ci[j] >> 40) >= (u64)a.min_count;
    }
    slot[j] = svo_compact_slot<VX_T>(keep, total, sW);
  }
  if (total == 0) return;  // workgroup-uniform
  if (threadIdx.x == 0) {
    const int base = __hip_atomic_fetch_add(&a.counts[0], total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // this workgroup's share of n_stored = min(n_total, max_points): the shares of all workgroups add up to it in any order
    const int lo = min(base, a.max_points), hi = min(base + total, a.max_points);
    if (hi > lo) __hip_atomic_fetch_add(&a.counts[1], hi - lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    sBase = base;
  }
  __syncthreads();
  const int base = sBase;
  const double vs = (double)a.voxel_size;
#pragma unroll
  for (int j = 0; j < VX_ITEMS; ++j) {
    if (slot[j] < 0 || base + slot[j] >= a.max_points) continue;
    const size_t s = first + (size_t)j * VX_T;
    const u64 key = a.t.keys[s];
    const u64 count = ci[j] >> 40, isum = ci[j] & ((1ull << 40) - 1ull);
    const u64 sum[3] = {a.t.sx[s], a.t.sy[s], a.t.sz[s]};
    float xyz[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) xyz[r] = (float)vx_mean(key, r, sum[r], count, vs);
    svo_cloud_point q;
    q.x = xyz[0]; q.y = xyz[1]; q.z = xyz[2];
    q.tag = (uint32_t)count | ((uint32_t)(isum / count) << 24);
    a.out[(size_t)(base + slot[j])] = q;
  }
}

__global__ __launch_bounds__(VX_T) void voxel_carve_kernel(VoxelCarveArgs a) {
  const size_t cap = (size_t)a.t.mask + 1;
  const size_t first = vx_walk_first();
  const double vs = (double)a.voxel_size;
  const double xlo = (double)a.radius, xhi = (double)(a.width - 1 - a.radius), yhi = (double)(a.height - 1 - a.radius);
  unsigned n_live = 0, n_tested = 0, n_carved = 0;
#pragma unroll
  for (int j = 0; j < VX_ITEMS; ++j) {
    const size_t s = first + (size_t)j * VX_T;
    if (s >= cap) continue;
    const u64 key = a.t.keys[s];
    if (key == VX_EMPTY) continue;
    const u64 count = a.t.ci[s] >> 40;
    if (count == 0) continue;
    ++n_live;
    const u64 sum[3] = {a.t.sx[s], a.t.sy[s], a.t.sz[s]};
    double p[3], q[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) p[r] = vx_mean(key, r, sum[r], count, vs);
#pragma unroll
    for (int r = 0; r < 3; ++r) q[r] = vx_to_camera(a, r, p);
    if (!(q[2] > 0.0)) continue;
    const double fpx = vx_pixel(a.focal, q[0], q[2], a.cx), fpy = vx_pixel(a.focal, q[1], q[2], a.cy);
    if (!(fpx >= xlo && fpx <= xhi && fpy >= xlo && fpy <= yhi)) continue;  // NaN and infinity fail
    ++n_tested;
    const int px = (int)fpx, py = (int)fpy;  // inside the map with the whole window, by the test above
    int dmax = 0;
    bool evidence = true;
    for (int dy = -a.radius; dy <= a.radius; ++dy) {
      const int16_t* row = a.disp + (size_t)(py + dy) * (size_t)a.width + (size_t)px;
      for (int dx = -a.radius; dx <= a.radius; ++dx) {
        const int d = (int)row[dx];
        evidence = evidence && d > 0;
        dmax = d > dmax ? d : dmax;
      }
    }
    if (!evidence) continue;
    const double dv16 = a.focal * a.baseline / q[2] * 16.0;
    if (!((double)(dmax + a.margin16) < dv16)) continue;
    if (a.keep_count > 0u && count >= (u64)a.keep_count) continue;
    a.t.ci[s] = 0ull; a.t.sx[s] = 0ull; a.t.sy[s] = 0ull; a.t.sz[s] = 0ull;
    ++n_carved;
  }
  if (!a.counts) return;  // uniform over the launch
  unsigned n[3] = {n_live, n_tested, n_carved};
  vx_wave_sum(n);
  vx_tally(n, a.counts);
}

__global__ __launch_bounds__(VX_T) void voxel_copy_kernel(VoxelCopyArgs a) {
  const size_t cap = (size_t)a.src.mask + 1;
  const size_t first = vx_walk_first();
  u64 n_claim = 0, n_moved = 0, n_drop = 0;  // a slot's count is below 2^24, a workgroup's 2,048 slots sum past 32 bits
#pragma unroll
  for (int j = 0; j < VX_ITEMS; ++j) {
    const size_t s = first + (size_t)j * VX_T;
    if (s >= cap) continue;
    const u64 key = a.src.keys[s];
    if (key == VX_EMPTY) continue;
    const u64 ci = a.src.ci[s], count = ci >> 40;
    if (count < (u64)a.min_count) continue;
    if (a.boxed) {
      bool in = true;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const int k = (int)((key >> (21 * r)) & 0x1FFFFFull) - (1 << 20);
        in = in && k >= a.klo[r] && k <= a.khi[r];
      }
      if (!in) continue;
    }
    u64 h;
    const int got = vx_probe(a.dst, key, h);
    if (got) {
      vx_add(a.dst, h, ci, a.src.sx[s], a.src.sy[s], a.src.sz[s]);
      n_claim += got == 2 ? 1ull : 0ull;
      n_moved += count;
    } else {
      n_drop += count;
    }
  }
  // vx_wave_sum and vx_tally written out, in u64: through them this kernel's three runs were slower than all five of the parent's
  // on one map (73.1, 70.4, 70.1 us against 69.0 .. 69.8) and above their middle on two more (profiles/voxel_written_once.txt).
  __shared__ u64 sC[3][VX_T / 64];
  for (int o = 32; o > 0; o >>= 1) {
    n_claim += __shfl_xor(n_claim, o); n_moved += __shfl_xor(n_moved, o); n_drop += __shfl_xor(n_drop, o);
  }
  const int tid = threadIdx.x;
  if ((tid & 63) == 0) { sC[0][tid >> 6] = n_claim; sC[1][tid >> 6] = n_moved; sC[2][tid >> 6] = n_drop; }
  __syncthreads();
  if (tid < 3) {
    u64 t = 0;
    for (int w = 0; w < VX_T / 64; ++w) t += sC[tid][w];  // counters: n_voxels, n_inserted, (n_rejected), n_dropped
    if (t) __hip_atomic_fetch_add(&a.dst.counters[tid == 2 ? 3 : tid], t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// One pixel of a footprint.
template <bool PRE>
__device__ __forceinline__ void vx_splat_max(unsigned* p, unsigned v) {
  if (PRE && *p >= v) return;
  __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <bool PRE, bool COOP>
__global__ __launch_bounds__(VX_T) void voxel_splat_kernel(VoxelSplatArgs a) {
  const size_t cap = (size_t)a.t.mask + 1;
  const size_t first = vx_walk_first();
  const int lane = threadIdx.x & 63;
  const double vs = (double)a.voxel_size, rmax = (double)a.max_radius;
  const double xhi = (double)(a.width - 1), yhi = (double)(a.height - 1);
  unsigned n_qual = 0, n_drawn = 0, n_splat = 0;
#pragma unroll
  for (int j = 0; j < VX_ITEMS; ++j) {  // no lane leaves the loop early: the ballot below is the whole wavefront's
    const size_t s = first + (size_t)j * VX_T;
    int px = 0, py = 0, r = -1;  // r >= 0: drawn
    unsigned v = 0;
    if (s < cap) {
      const u64 key = a.t.keys[s];
      if (key != VX_EMPTY) {
        const u64 ci = a.t.ci[s], count = ci >> 40;
        if (count >= (u64)a.min_count) {
          ++n_qual;
          const u64 sum[3] = {a.t.sx[s], a.t.sy[s], a.t.sz[s]};
          double p[3], q[3];
#pragma unroll
          for (int k3 = 0; k3 < 3; ++k3) p[k3] = vx_mean(key, k3, sum[k3], count, vs);
#pragma unroll
          for (int k3 = 0; k3 < 3; ++k3) q[k3] = vx_to_camera(a, k3, p);
          if (q[2] > 0.0) {
            const double fpx = vx_pixel(a.focal, q[0], q[2], a.cx), fpy = vx_pixel(a.focal, q[1], q[2], a.cy);
            const double d16 = floor(a.focal * a.baseline / q[2] * 16.0 + 0.5);
            const double h = floor(a.focal * vs / q[2] * 0.5 + 0.5);
            const double fr = h < rmax ? h : rmax;
            // NaN and infinity fail
            if (d16 >= 1.0 && d16 <= 32767.0 && fpx >= -fr && fpx <= xhi + fr && fpy >= -fr && fpy <= yhi + fr) {
              ++n_drawn;
              px = (int)fpx; py = (int)fpy; r = (int)fr;
              v = ((unsigned)d16 << 8) | (unsigned)((ci & ((1ull << 40) - 1ull)) / count);
            }
          }
        }
      }
    }
    if (r >= 0) {  // the footprint clipped to the image: not empty, by the test above
      const int x0 = max(px - r, 0), x1 = min(px + r, a.width - 1), y0 = max(py - r, 0), y1 = min(py + r, a.height - 1);
      n_splat += (unsigned)((x1 - x0 + 1) * (y1 - y0 + 1));
      if (!COOP || r <= 1) {
        for (int y = y0; y <= y1; ++y) {
          unsigned* row = a.pix + (size_t)y * (size_t)a.width;
          for (int x = x0; x <= x1; ++x) vx_splat_max<PRE>(row + x, v);
        }
      }
    }
    if (COOP) {
      u64 todo = __ballot(r > 1);
      while (todo) {  // wavefront-uniform
        const int src = __builtin_ctzll(todo);
        todo &= todo - 1ull;
        const int bx = __shfl(px, src), by = __shfl(py, src), br = __shfl(r, src);
        const unsigned bv = __shfl(v, src);
        const int x0 = max(bx - br, 0), x1 = min(bx + br, a.width - 1), y0 = max(by - br, 0), y1 = min(by + br, a.height - 1);
        const int bw = x1 - x0 + 1, n = bw * (y1 - y0 + 1);  // 1 <= bw <= 33
        const int sy = 64 / bw, sx = 64 - sy * bw;           // one step of 64 pixels in rows and columns
        int yy = lane / bw, xx = lane - yy * bw;
        for (int i = lane; i < n; i += 64) {
          vx_splat_max<PRE>(a.pix + (size_t)(y0 + yy) * (size_t)a.width + (size_t)(x0 + xx), bv);
          yy += sy; xx += sx;
          if (xx >= bw) { xx -= bw; ++yy; }
        }
      }
    }
  }
  if (!a.counts) return;  // uniform over the launch
  unsigned n[3] = {n_qual, n_drawn, n_splat};
  vx_wave_sum(n);
  vx_tally(n, a.counts);
}

__global__ __launch_bounds__(VX_T) void voxel_resolve_kernel(VoxelResolveArgs a) {
  const size_t i0 = ((size_t)blockIdx.x * VX_T + (size_t)threadIdx.x) * 4;
  const int here = i0 < a.n ? (int)(a.n - i0 < 4 ? a.n - i0 : 4) : 0;
  unsigned covered = 0;  // one bit per pixel
  if (here == 4 && a.vec) {
    const uint4 p = *reinterpret_cast<const uint4*>(a.pix + i0);
    covered = (p.x ? 1u : 0u) | (p.y ? 2u : 0u) | (p.z ? 4u : 0u) | (p.w ? 8u : 0u);
    short4 d;
    d.x = p.x ? (short)(p.x >> 8) : (short)-16; d.y = p.y ? (short)(p.y >> 8) : (short)-16;
    d.z = p.z ? (short)(p.z >> 8) : (short)-16; d.w = p.w ? (short)(p.w >> 8) : (short)-16;
    *reinterpret_cast<short4*>(a.disp + i0) = d;
    if (a.inten) {
      uchar4 g;
      g.x = (unsigned char)(p.x & 255u); g.y = (unsigned char)(p.y & 255u); g.z = (unsigned char)(p.z & 255u); g.w = (unsigned char)(p.w & 255u);
      *reinterpret_cast<uchar4*>(a.inten + i0) = g;
    }
  } else {
    for (int k = 0; k < here; ++k) {  // the tail, or pointers the vector form cannot take
      const unsigned p = a.pix[i0 + k];
      covered |= p ? 1u << k : 0u;
      a.disp[i0 + k] = p ? (int16_t)(p >> 8) : (int16_t)-16;
      if (a.inten) a.inten[i0 + k] = (uint8_t)(p & 255u);
    }
  }
  if (!a.counts) return;  // uniform over the launch
  unsigned n[1] = {(unsigned)__popc(covered)};
  vx_wave_sum(n);
  vx_tally(n, a.counts + 3);  // n_pixels
}

// The signed index of one axis in a key.
__device__ __forceinline__ int vx_key_index(u64 key, int shift) { return (int)((key >> shift) & 0x1FFFFFull) - (1 << 20); }

// One of a cell's two max words.  PRE: a relaxed device-scope load skips the atomic where the word already holds at least the value.
// Words only grow within the launch and the memset precedes it on the stream, so a stale load costs a needless atomic, never a
// wrong skip: no bit of the grid depends on PRE (svo_voxel_grid_set_mode).
template <bool PRE>
__device__ __forceinline__ void vx_grid_max(u64* p, u64 v) {
  if (PRE && __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= v) return;
  __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <bool PRE>
__global__ __launch_bounds__(VX_T) void voxel_grid_kernel(VoxelGridArgs a) {
  const size_t first = vx_walk_first();
  unsigned n_qual = 0, n_band = 0, n_bin = 0;
#pragma unroll
  for (int j = 0; j < VX_ITEMS; ++j) {
    const size_t s = first + (size_t)j * VX_T;
    if (s >= a.cap) continue;
    const u64 key = a.keys[s];
    if (key == VX_EMPTY) continue;
    const u64 ci = a.ci[s];
    const unsigned count = (unsigned)(ci >> 40);
    if (count < a.min_count) continue;  // min_count >= 1: a carved slot stops here, nothing divides by 0
    ++n_qual;
    const long long g = (long long)vx_key_index(key, a.shift_up) * 65536ll + (long long)voxel_div40(a.sup[s], count);
    const long long hgt = a.up_sign < 0 ? -g : g;
    if (hgt < a.hlo || hgt > a.hhi) continue;
    ++n_band;
    const int ia = voxel_floordiv(vx_key_index(key, a.shift_a) - a.ka0, a.cell_voxels);
    const int ib = voxel_floordiv(vx_key_index(key, a.shift_b) - a.kb0, a.cell_voxels);
    if (ia < 0 || ia >= a.na || ib < 0 || ib >= a.nb) continue;
    ++n_bin;
    u64* cell = a.cells + 4 * ((size_t)ia * (size_t)a.nb + (size_t)ib);  // inside the workspace by the test above
    const u64 top = ((u64)(hgt + (1ll << 37)) << 8) | voxel_div40(ci & ((1ull << 40) - 1ull), count);
    vx_grid_max<PRE>(&cell[0], top);
    vx_grid_max<PRE>(&cell[1], (u64)((1ll << 37) - hgt));
    __hip_atomic_fetch_add(&cell[2], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add(&cell[3], (u64)count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (!a.counts) return;  // uniform over the launch
  unsigned n[3] = {n_qual, n_band, n_bin};
  vx_wave_sum(n);
  vx_tally(n, a.counts);
}

__global__ __launch_bounds__(VX_T) void voxel_grid_resolve_kernel(VoxelGridResolveArgs a) {
  const size_t i = (size_t)blockIdx.x * VX_T + (size_t)threadIdx.x;
  unsigned n_cells = 0, n_obstacle = 0;
  if (i < a.n) {
    const u64* cell = a.cells + 4 * i;
    const u64 nvox = cell[2];
    uint8_t cls = SVO_VOXEL_GRID_UNKNOWN, inten = 0;
    float top = -__builtin_inff(), bottom = __builtin_inff();
    u64 npts = 0;
    if (nvox) {
      const u64 t = cell[0];
      const long long htop = (long long)(t >> 8) - (1ll << 37), hbot = (1ll << 37) - (long long)cell[1];
      const double vs = (double)a.voxel_size;
      cls = htop - hbot > a.step ? SVO_VOXEL_GRID_OBSTACLE : SVO_VOXEL_GRID_LEVEL;
      top = (float)((double)htop / 65536.0 * vs);
      bottom = (float)((double)hbot / 65536.0 * vs);
      inten = (uint8_t)(t & 255ull);
      npts = cell[3];
      n_cells = 1;
      n_obstacle = cls == SVO_VOXEL_GRID_OBSTACLE ? 1u : 0u;
    }
    a.o.cls[i] = cls;
    if (a.o.top) a.o.top[i] = top;
    if (a.o.bottom) a.o.bottom[i] = bottom;
    if (a.o.intensity) a.o.intensity[i] = inten;
    if (a.o.n_voxels) a.o.n_voxels[i] = (uint32_t)nvox;
    if (a.o.n_points) a.o.n_points[i] = npts;
  }
  if (!a.counts) return;  // uniform over the launch
  unsigned n[2] = {n_cells, n_obstacle};
  vx_wave_sum(n);
  vx_tally(n, a.counts + 3);  // n_cells, n_obstacle
}

// ----------------------------------------------------------------------------- host side
// The head of every pose7 entry: null refused under the entry's own name, then the matrix its matrix form takes.
static int voxel_pose7(svo_voxel_map* m, const double* pose7, void (*to_matrix)(const double*, double*), double* m12, const char* null_text) {
  if (!m) return SVO_ERR_INVALID;
  SVO_REQUIRE(m->ctx, pose7, null_text);
  to_matrix(pose7, m12);
  return SVO_OK;
}

extern "C" int svo_voxel_map_default_params(svo_voxel_map_params* params) {
  if (!params) return SVO_ERR_INVALID;
  params->voxel_size = 0.1f; params->capacity_log2 = 22; params->max_depth = 0.0f;
  return SVO_OK;
}

extern "C" int svo_voxel_map_bytes(const svo_voxel_map_params* params, size_t* bytes) { return voxel_table_bytes(params, bytes); }

extern "C" int svo_pose7_to_cam_to_world(const double* pose7, double* m12) {
  if (!pose7 || !m12) return SVO_ERR_INVALID;
  voxel_pose7_to_cam_to_world(pose7, m12);
  return SVO_OK;
}

extern "C" int svo_pose7_to_world_to_cam(const double* pose7, double* m12) {
  if (!pose7 || !m12) return SVO_ERR_INVALID;
  voxel_pose7_to_world_to_cam(pose7, m12);
  return SVO_OK;
}

static int voxel_clear(svo_voxel_map* m) {
  svo_ctx* ctx = m->ctx;
  SVO_HIP_CHECK(ctx, hipMemsetAsync(m->t.keys, 0xFF, 8 * m->cap, ctx->stream));
  SVO_HIP_CHECK(ctx, hipMemsetAsync(m->t.ci, 0, 32 * m->cap + 4 * sizeof(u64) + 2 * sizeof(int), ctx->stream));
  return SVO_OK;
}

extern "C" int svo_voxel_map_create(svo_ctx* ctx, const svo_voxel_map_params* params, svo_voxel_map** out) {
  if (!ctx) return SVO_ERR_INVALID;
  svo_use_device(ctx);
  SVO_REQUIRE(ctx, out, "voxel_map_create: null out");
  *out = nullptr;
  SVO_ARGS_CHECK(ctx, voxel_params_check(params, &err));
  svo_voxel_map* m = new svo_voxel_map();
  m->ctx = ctx;
  m->prm = *params;
  m->cap = (size_t)1 << params->capacity_log2;
  const hipError_t e = hipMalloc((void**)&m->d_mem, VOXEL_SLOT_BYTES * m->cap + 4 * sizeof(u64) + 2 * sizeof(int));
  if (e != hipSuccess) {
    ctx->err = std::string("voxel_map_create: hipMalloc of the table: ") + hipGetErrorString(e);
    delete m;
    return SVO_ERR_HIP;
  }
  m->t.keys = m->d_mem;
  m->t.ci = m->d_mem + m->cap; m->t.sx = m->d_mem + 2 * m->cap; m->t.sy = m->d_mem + 3 * m->cap; m->t.sz = m->d_mem + 4 * m->cap;
  m->t.counters = m->d_mem + 5 * m->cap;
  m->t.mask = (u64)m->cap - 1;
  m->d_counts = reinterpret_cast<int*>(m->t.counters + 4);
  const int rc = voxel_clear(m);
  if (rc) { (void)hipFree(m->d_mem); delete m; return rc; }
  *out = m;
  return SVO_OK;
}

extern "C" void svo_voxel_map_destroy(svo_voxel_map* m) {
  if (!m) return;
  svo_use_device(m->ctx);
  (void)hipStreamSynchronize(m->ctx->stream);
  (void)hipFree(m->d_mem);
  delete m;
}

extern "C" int svo_voxel_map_clear(svo_voxel_map* m) {
  if (!m) return SVO_ERR_INVALID;
  svo_use_device(m->ctx);
  return voxel_clear(m);
}

SvoVoxelView svo_voxel_map_view(const svo_voxel_map* m) {  // kernels.h: for csrc/voxel_align.hip
  return SvoVoxelView{m->ctx, m->t.keys, m->t.ci, m->t.sx, m->t.sy, m->t.sz, m->t.mask, m->prm.voxel_size, m->prm.max_depth};
}

static int voxel_insert_launch(svo_voxel_map* m, const svo_cloud_point* points, int n, const double* m12) {
  svo_ctx* ctx = m->ctx;
  VoxelInsertArgs a{};
  a.pts = points; a.n = n; a.t = m->t;
  memcpy(a.m, m12, sizeof(a.m));
  a.voxel_size = m->prm.voxel_size; a.max_depth = m->prm.max_depth;
  hipLaunchKernelGGL(voxel_insert_kernel, dim3((unsigned)voxel_record_groups(n)), dim3(VX_T), 0, ctx->stream, a);
  SVO_HIP_CHECK(ctx, hipGetLastError());
  return SVO_OK;
}

extern "C" int svo_voxel_map_insert_dev(svo_voxel_map* m, const svo_cloud_point* points, int n, const double* m12) {
  if (!m) return SVO_ERR_INVALID;
  svo_ctx* ctx = m->ctx;
  svo_use_device(ctx);
  SVO_ARGS_CHECK(ctx, voxel_cloud_check(points, n, m12, VOXEL_INSERT_TEXTS, &err));
  if (n == 0) return SVO_OK;
  SvoProfScope prof(ctx, SVO_PROF_VOXEL_INSERT);
  return voxel_insert_launch(m, points, n, m12);
}

extern "C" int svo_voxel_map_insert_pose7_dev(svo_voxel_map* m, const svo_cloud_point* points, int n, const double* pose7) {
  double m12[12];
  const int rc = voxel_pose7(m, pose7, voxel_pose7_to_cam_to_world, m12, "voxel_map_insert_pose7: null pose7");
  return rc ? rc : svo_voxel_map_insert_dev(m, points, n, m12);
}

extern "C" int svo_voxel_map_stats(svo_voxel_map* m, svo_voxel_map_stats_t* stats) {
  if (!m) return SVO_ERR_INVALID;
  svo_ctx* ctx = m->ctx;
  svo_use_device(ctx);
  SVO_REQUIRE(ctx, stats, "voxel_map_stats: null stats");
  u64 c[4] = {0, 0, 0, 0};
  SVO_HIP_CHECK(ctx, hipMemcpyAsync(c, m->t.counters, sizeof(c), hipMemcpyDeviceToHost, ctx->stream));
  SVO_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  stats->n_voxels = c[0]; stats->n_inserted = c[1]; stats->n_rejected = c[2]; stats->n_dropped = c[3];
  return SVO_OK;
}

extern "C" int svo_voxel_map_extract_dev(svo_voxel_map* m, int min_count, svo_cloud_point* points, int max_points, int* counts) {
  if (!m) return SVO_ERR_INVALID;
  svo_ctx* ctx = m->ctx;
  svo_use_device(ctx);
  SVO_REQUIRE(ctx, min_count >= 1, "voxel_map_extract: min_count must be at least 1");
  SVO_REQUIRE(ctx, max_points >= 0, "voxel_map_extract: max_points must not be negative");
  SVO_REQUIRE(ctx, points || max_points == 0, "voxel_map_extract: null points");
  SVO_REQUIRE(ctx, counts, "voxel_map_extract: null counts");
  VoxelExtractArgs a{};
  a.t = m->t;
  a.min_count = (unsigned)min_count;
  a.voxel_size = m->prm.voxel_size;
  a.out = points; a.max_points = max_points; a.counts = counts;
  SvoProfScope prof(ctx, SVO_PROF_VOXEL_EXTRACT);
  SVO_HIP_CHECK(ctx, hipMemsetAsync(counts, 0, 2 * sizeof(int), ctx->stream));
  hipLaunchKernelGGL(voxel_extract_kernel, dim3((unsigned)voxel_walk_groups(m->cap)), dim3(VX_T), 0, ctx->stream, a);
  SVO_HIP_CHECK(ctx, hipGetLastError());
  return SVO_OK;
}

extern "C" int svo_voxel_map_extract(svo_voxel_map* m, int min_count, svo_cloud_point* points, int capacity, int* n_total, int* n_stored) {
  if (!m) return SVO_ERR_INVALID;
  svo_ctx* ctx = m->ctx;
  svo_use_device(ctx);
  SVO_REQUIRE(ctx, min_count >= 1, "voxel_map_extract: min_count must be at least 1");
  SVO_REQUIRE(ctx, capacity >= 0, "voxel_map_extract: capacity must not be negative");
  SVO_REQUIRE(ctx, points || capacity == 0, "voxel_map_extract: null points");
  SVO_REQUIRE(ctx, n_total && n_stored, "voxel_map_extract: null n_total or n_stored");
  const size_t room = (size_t)capacity < m->cap ? (size_t)capacity : m->cap;  // no more than cap voxels exist
  SvoTemp hold;
  if (room) SVO_HIP_CHECK(ctx, hipMalloc(&hold.p, room * sizeof(svo_cloud_point)));
  svo_cloud_point* const d = hold.at<svo_cloud_point>(0);
  int c[2] = {0, 0};
  const int rc = svo_host_call(
      ctx, "voxel_map_extract", hipSuccess, [&] { return svo_voxel_map_extract_dev(m, min_count, d, (int)room, m->d_counts); },
      [&] {  // the counts first: they say how many points there are to copy
        hipError_t e = hipMemcpyAsync(c, m->d_counts, sizeof(c), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess && c[1] > 0) e = hipMemcpyAsync(points, d, sizeof(svo_cloud_point) * (size_t)c[1], hipMemcpyDeviceToHost, ctx->stream);
        return e;
      });
  if (rc) return rc;
  *n_total = c[0]; *n_stored = c[1];
  return SVO_OK;
}

extern "C" int svo_voxel_map_download(svo_voxel_map* m, void* host, size_t bytes) {
  if (!m) return SVO_ERR_INVALID;
  svo_ctx* ctx = m->ctx;
  svo_use_device(ctx);
  SVO_REQUIRE(ctx, host, "voxel_map_download: null host buffer");
  SVO_REQUIRE(ctx, bytes >= VOXEL_SLOT_BYTES * m->cap, "voxel_map_download: bytes is less than svo_voxel_map_bytes");
  SVO_HIP_CHECK(ctx, hipMemcpyAsync(host, m->d_mem, VOXEL_SLOT_BYTES * m->cap, hipMemcpyDeviceToHost, ctx->stream));
  SVO_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return SVO_OK;
}

// ----------------------------------------------------------------------------- carving and the copy of the live voxels
extern "C" int svo_voxel_carve_default_params(svo_voxel_carve_params* params) {
  if (!params) return SVO_ERR_INVALID;
  params->radius = 1; params->margin16 = 8; params->keep_count = 0;
  return SVO_OK;
}

extern "C" int svo_voxel_map_carve_dev(svo_voxel_map* m, const int16_t* disp16, int width, int height, const svo_camera_info* cam,
                                       const double* w2c12, const svo_voxel_carve_params* prm, uint64_t* counts) {
  if (!m) return SVO_ERR_INVALID;
  svo_ctx* ctx = m->ctx;
  svo_use_device(ctx);
  SVO_ARGS_CHECK(ctx, voxel_carve_check(disp16, width, height, cam, w2c12, prm, ctx->lim.max_width, ctx->lim.max_height, &err));
  VoxelCarveArgs a{};
  a.t = m->t;
  a.disp = disp16; a.width = width; a.height = height;
  a.radius = prm->radius; a.margin16 = prm->margin16; a.keep_count = (unsigned)prm->keep_count;
  a.voxel_size = m->prm.voxel_size;
  memcpy(a.m, w2c12, sizeof(a.m));
  a.focal = cam->focal; a.cx = cam->cx; a.cy = cam->cy; a.baseline = cam->baseline;
  a.counts = reinterpret_cast<u64*>(counts);
  SvoProfScope prof(ctx, SVO_PROF_VOXEL_CARVE);
  if (counts) SVO_HIP_CHECK(ctx, hipMemsetAsync(counts, 0, 3 * sizeof(u64), ctx->stream));
  hipLaunchKernelGGL(voxel_carve_kernel, dim3((unsigned)voxel_walk_groups(m->cap)), dim3(VX_T), 0, ctx->stream, a);
  SVO_HIP_CHECK(ctx, hipGetLastError());
  return SVO_OK;
}

extern "C" int svo_voxel_map_carve_pose7_dev(svo_voxel_map* m, const int16_t* disp16, int width, int height, const svo_camera_info* cam,
                                             const double* pose7, const svo_voxel_carve_params* prm, uint64_t* counts) {
  double m12[12];
  const int rc = voxel_pose7(m, pose7, voxel_pose7_to_world_to_cam, m12, "voxel_map_carve_pose7: null pose7");
  return rc ? rc : svo_voxel_map_carve_dev(m, disp16, width, height, cam, m12, prm, counts);
}

extern "C" int svo_voxel_map_carve(svo_voxel_map* m, const int16_t* disp16, int width, int height, const svo_camera_info* cam,
                                   const double* w2c12, const svo_voxel_carve_params* prm, uint64_t* counts) {
  if (!m) return SVO_ERR_INVALID;
  svo_ctx* ctx = m->ctx;
  svo_use_device(ctx);
  SVO_ARGS_CHECK(ctx, voxel_carve_check(disp16, width, height, cam, w2c12, prm, ctx->lim.max_width, ctx->lim.max_height, &err));
  const size_t bytes = sizeof(int16_t) * (size_t)width * (size_t)height;
  SvoParts parts;
  const size_t o_counts = parts.add(3 * sizeof(u64)), o_disp = parts.add(bytes);
  SvoTemp hold;
  SVO_HIP_CHECK(ctx, hipMalloc(&hold.p, parts.total()));
  u64* const d = hold.at<u64>(o_counts);
  int16_t* const d_disp = hold.at<int16_t>(o_disp);
  u64 c[3] = {0, 0, 0};
  const int rc = svo_host_call(
      ctx, "voxel_map_carve", hipMemcpyAsync(d_disp, disp16, bytes, hipMemcpyHostToDevice, ctx->stream),
      [&] { return svo_voxel_map_carve_dev(m, d_disp, width, height, cam, w2c12, prm, reinterpret_cast<uint64_t*>(d)); },
      [&] { return hipMemcpyAsync(c, d, sizeof(c), hipMemcpyDeviceToHost, ctx->stream); });
  if (rc) return rc;
  if (counts) { counts[0] = c[0]; counts[1] = c[1]; counts[2] = c[2]; }
  return SVO_OK;
}

extern "C" int svo_voxel_map_copy_live_dev(svo_voxel_map* src, svo_voxel_map* dst, int min_count, const double* box6) {
  if (!src || !dst) return SVO_ERR_INVALID;
  svo_ctx* ctx = dst->ctx;
  svo_use_device(ctx);
  SVO_REQUIRE(ctx, src != dst, "voxel_map_copy_live: src and dst are the same map");
  SVO_REQUIRE(ctx, src->ctx == dst->ctx, "voxel_map_copy_live: src and dst belong to different contexts");
  SVO_REQUIRE(ctx, memcmp(&src->prm.voxel_size, &dst->prm.voxel_size, sizeof(float)) == 0, "voxel_map_copy_live: voxel_size of src and dst differ");
  SVO_REQUIRE(ctx, min_count >= 1, "voxel_map_copy_live: min_count must be at least 1");
  VoxelCopyArgs a{};
  a.src = src->t; a.dst = dst->t;
  a.min_count = (unsigned)min_count;
  if (box6) {
    SVO_ARGS_CHECK(ctx, voxel_box_keys(box6, src->prm.voxel_size, a.klo, a.khi, &err));
    a.boxed = 1;
  }
  SvoProfScope prof(ctx, SVO_PROF_VOXEL_COPY);
  hipLaunchKernelGGL(voxel_copy_kernel, dim3((unsigned)voxel_walk_groups(src->cap)), dim3(VX_T), 0, ctx->stream, a);
  SVO_HIP_CHECK(ctx, hipGetLastError());
  return SVO_OK;
}

// ----------------------------------------------------------------------------- the render
extern "C" int svo_voxel_render_default_params(svo_voxel_render_params* params) {
  if (!params) return SVO_ERR_INVALID;
  params->min_count = 1; params->max_radius = 8;
  return SVO_OK;
}

extern "C" size_t svo_voxel_render_workspace_bytes(int width, int height) {
  return width < 1 || height < 1 ? 0 : 4 * (size_t)width * (size_t)height;
}

extern "C" int svo_voxel_render_set_mode(svo_voxel_map* m, int cooperative, int precheck) {
  if (!m) return SVO_ERR_INVALID;
  m->render_coop = cooperative != 0; m->render_pre = precheck != 0;
  return SVO_OK;
}

// The splat launch's four forms, [cooperative][pre-check] (svo_voxel_render_set_mode).
static void (*const voxel_splat_form[2][2])(VoxelSplatArgs) = {{voxel_splat_kernel<false, false>, voxel_splat_kernel<true, false>},
                                                               {voxel_splat_kernel<false, true>, voxel_splat_kernel<true, true>}};

extern "C" int svo_voxel_map_render_dev(svo_voxel_map* m, int width, int height, const svo_camera_info* cam, const double* w2c12,
                                        const svo_voxel_render_params* prm, void* workspace, int16_t* disp16, uint8_t* intensity,
                                        uint64_t* counts) {
  if (!m) return SVO_ERR_INVALID;
  svo_ctx* ctx = m->ctx;
  svo_use_device(ctx);
  SVO_ARGS_CHECK(ctx, voxel_render_check(width, height, cam, w2c12, prm, ctx->lim.max_width, ctx->lim.max_height, &err));
  SVO_REQUIRE(ctx, workspace, "voxel_map_render: null workspace");
  SVO_REQUIRE(ctx, ((uintptr_t)workspace & 3u) == 0, "voxel_map_render: workspace must be 4-byte aligned");
  SVO_REQUIRE(ctx, disp16, "voxel_map_render: null disp16");
  VoxelSplatArgs a{};
  a.t = m->t;
  a.pix = static_cast<unsigned*>(workspace);
  a.width = width; a.height = height; a.max_radius = prm->max_radius;
  a.min_count = (unsigned)prm->min_count;
  a.voxel_size = m->prm.voxel_size;
  memcpy(a.m, w2c12, sizeof(a.m));
  a.focal = cam->focal; a.cx = cam->cx; a.cy = cam->cy; a.baseline = cam->baseline;
  a.counts = reinterpret_cast<u64*>(counts);
  VoxelResolveArgs b{};
  b.pix = a.pix; b.disp = disp16; b.inten = intensity;
  b.n = (size_t)width * (size_t)height;
  b.vec = voxel_resolve_vector_ok(workspace, disp16, intensity);
  b.counts = a.counts;
  SvoProfScope prof(ctx, SVO_PROF_VOXEL_RENDER);
  SVO_HIP_CHECK(ctx, hipMemsetAsync(workspace, 0, 4 * b.n, ctx->stream));
  if (counts) SVO_HIP_CHECK(ctx, hipMemsetAsync(counts, 0, 4 * sizeof(u64), ctx->stream));
  hipLaunchKernelGGL(voxel_splat_form[m->render_coop][m->render_pre], dim3((unsigned)voxel_walk_groups(m->cap)), dim3(VX_T), 0, ctx->stream, a);
  SVO_HIP_CHECK(ctx, hipGetLastError());
  hipLaunchKernelGGL(voxel_resolve_kernel, dim3((unsigned)voxel_resolve_groups(b.n)), dim3(VX_T), 0, ctx->stream, b);
  SVO_HIP_CHECK(ctx, hipGetLastError());
  return SVO_OK;
}

extern "C" int svo_voxel_map_render_pose7_dev(svo_voxel_map* m, int width, int height, const svo_camera_info* cam, const double* pose7,
                                              const svo_voxel_render_params* prm, void* workspace, int16_t* disp16, uint8_t* intensity,
                                              uint64_t* counts) {
  double m12[12];
  const int rc = voxel_pose7(m, pose7, voxel_pose7_to_world_to_cam, m12, "voxel_map_render_pose7: null pose7");
  return rc ? rc : svo_voxel_map_render_dev(m, width, height, cam, m12, prm, workspace, disp16, intensity, counts);
}

extern "C" int svo_voxel_map_render(svo_voxel_map* m, int width, int height, const svo_camera_info* cam, const double* w2c12,
                                    const svo_voxel_render_params* prm, int16_t* disp16, uint8_t* intensity, uint64_t* counts) {
  if (!m) return SVO_ERR_INVALID;
  svo_ctx* ctx = m->ctx;
  svo_use_device(ctx);
  SVO_ARGS_CHECK(ctx, voxel_render_check(width, height, cam, w2c12, prm, ctx->lim.max_width, ctx->lim.max_height, &err));
  SVO_REQUIRE(ctx, disp16, "voxel_map_render: null disp16");
  const size_t n = (size_t)width * (size_t)height;
  SvoParts parts;
  const size_t o_counts = parts.add(4 * sizeof(u64)), o_pix = parts.add(svo_voxel_render_workspace_bytes(width, height)), o_disp = parts.add(2 * n),
               o_int = parts.add(n);
  SvoTemp hold;
  SVO_HIP_CHECK(ctx, hipMalloc(&hold.p, parts.total()));
  u64* const d = hold.at<u64>(o_counts);
  unsigned char* const d_pix = hold.at(o_pix);
  int16_t* const d_disp = hold.at<int16_t>(o_disp);
  uint8_t* const d_int = hold.at(o_int);
  u64 c[4] = {0, 0, 0, 0};
  const int rc = svo_host_call(
      ctx, "voxel_map_render", hipSuccess,
      [&] { return svo_voxel_map_render_dev(m, width, height, cam, w2c12, prm, d_pix, d_disp, intensity ? d_int : nullptr, reinterpret_cast<uint64_t*>(d)); },
      [&] {
        hipError_t e = hipMemcpyAsync(disp16, d_disp, sizeof(int16_t) * n, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess && intensity) e = hipMemcpyAsync(intensity, d_int, n, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(c, d, sizeof(c), hipMemcpyDeviceToHost, ctx->stream);
        return e;
      });
  if (rc) return rc;
  if (counts) for (int i = 0; i < 4; ++i) counts[i] = c[i];
  return SVO_OK;
}

// ----------------------------------------------------------------------------- the grid
extern "C" int svo_voxel_grid_default_params(float voxel_size, svo_voxel_grid_params* params) { return voxel_grid_default_params(voxel_size, params); }

extern "C" size_t svo_voxel_grid_workspace_bytes(int na, int nb) { return voxel_grid_workspace_bytes(na, nb); }

extern "C" int svo_voxel_grid_cell_of(const svo_voxel_grid_params* params, float voxel_size, double a, double b, int* ia, int* ib) {
  return voxel_grid_cell_of(params, voxel_size, a, b, ia, ib);
}

extern "C" int svo_voxel_grid_set_mode(svo_voxel_map* m, int precheck) {
  if (!m) return SVO_ERR_INVALID;
  m->grid_pre = precheck != 0;
  return SVO_OK;
}

// The walk's two forms, [pre-check] (svo_voxel_grid_set_mode).
static void (*const voxel_grid_form[2])(VoxelGridArgs) = {voxel_grid_kernel<false>, voxel_grid_kernel<true>};

extern "C" int svo_voxel_map_grid_dev(svo_voxel_map* m, const svo_voxel_grid_params* prm, void* workspace, const svo_voxel_grid_out* out,
                                      uint64_t* counts) {
  if (!m) return SVO_ERR_INVALID;
  svo_ctx* ctx = m->ctx;
  svo_use_device(ctx);
  SVO_ARGS_CHECK(ctx, voxel_grid_check(prm, workspace, out, counts, &err));
  VoxelGridKeys k;
  voxel_grid_keys(prm, m->prm.voxel_size, &k);
  const u64* const sums[3] = {m->t.sx, m->t.sy, m->t.sz};
  VoxelGridArgs a{};
  a.keys = m->t.keys; a.ci = m->t.ci; a.sup = sums[prm->up_axis];
  a.cap = m->cap;
  a.cells = static_cast<u64*>(workspace);
  a.shift_up = 21 * prm->up_axis; a.shift_a = 21 * ((prm->up_axis + 1) % 3); a.shift_b = 21 * ((prm->up_axis + 2) % 3);
  a.up_sign = prm->up_sign; a.ka0 = k.ka0; a.kb0 = k.kb0; a.cell_voxels = prm->cell_voxels; a.na = prm->na; a.nb = prm->nb;
  a.min_count = (unsigned)prm->min_count;
  a.hlo = k.hlo; a.hhi = k.hhi;
  a.counts = reinterpret_cast<u64*>(counts);
  VoxelGridResolveArgs b{};
  b.cells = a.cells;
  b.n = (size_t)prm->na * (size_t)prm->nb;
  b.step = k.step;
  b.voxel_size = m->prm.voxel_size;
  b.o = *out;
  b.counts = a.counts;
  SvoProfScope prof(ctx, SVO_PROF_VOXEL_GRID);
  SVO_HIP_CHECK(ctx, hipMemsetAsync(workspace, 0, voxel_grid_workspace_bytes(prm->na, prm->nb), ctx->stream));
  if (counts) SVO_HIP_CHECK(ctx, hipMemsetAsync(counts, 0, 5 * sizeof(u64), ctx->stream));
  hipLaunchKernelGGL(voxel_grid_form[m->grid_pre], dim3((unsigned)voxel_walk_groups(m->cap)), dim3(VX_T), 0, ctx->stream, a);
  SVO_HIP_CHECK(ctx, hipGetLastError());
  hipLaunchKernelGGL(voxel_grid_resolve_kernel, dim3((unsigned)voxel_grid_resolve_groups(b.n)), dim3(VX_T), 0, ctx->stream, b);
  SVO_HIP_CHECK(ctx, hipGetLastError());
  return SVO_OK;
}

extern "C" int svo_voxel_map_grid(svo_voxel_map* m, const svo_voxel_grid_params* prm, const svo_voxel_grid_out* out, uint64_t* counts) {
  if (!m) return SVO_ERR_INVALID;
  svo_ctx* ctx = m->ctx;
  svo_use_device(ctx);
  SVO_ARGS_CHECK(ctx, voxel_grid_params_check(prm, &err));
  SVO_ARGS_CHECK(ctx, voxel_grid_out_check(out, false, &err));
  const size_t n = (size_t)prm->na * (size_t)prm->nb;
  SvoParts parts;
  const size_t o_counts = parts.add(5 * sizeof(u64)), o_cells = parts.add(voxel_grid_workspace_bytes(prm->na, prm->nb)), o_points = parts.add(8 * n),
               o_top = parts.add(4 * n), o_bottom = parts.add(4 * n), o_voxels = parts.add(4 * n), o_cls = parts.add(n), o_int = parts.add(n);
  SvoTemp hold;
  SVO_HIP_CHECK(ctx, hipMalloc(&hold.p, parts.total()));
  u64* const d = hold.at<u64>(o_counts);
  unsigned char* const d_cells = hold.at(o_cells);
  svo_voxel_grid_out o{};
  o.n_points = hold.at<uint64_t>(o_points);
  o.top = hold.at<float>(o_top);
  o.bottom = hold.at<float>(o_bottom);
  o.n_voxels = hold.at<uint32_t>(o_voxels);
  o.cls = hold.at(o_cls);
  o.intensity = hold.at(o_int);
  svo_voxel_grid_out asked = o;  // what the caller did not ask for is not written
  if (!out->top) asked.top = nullptr;
  if (!out->bottom) asked.bottom = nullptr;
  if (!out->intensity) asked.intensity = nullptr;
  if (!out->n_voxels) asked.n_voxels = nullptr;
  if (!out->n_points) asked.n_points = nullptr;
  u64 c[5] = {0, 0, 0, 0, 0};
  const int rc = svo_host_call(
      ctx, "voxel_map_grid", hipSuccess, [&] { return svo_voxel_map_grid_dev(m, prm, d_cells, &asked, reinterpret_cast<uint64_t*>(d)); },
      [&] {
        hipError_t e = hipMemcpyAsync(out->cls, o.cls, n, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess && out->top) e = hipMemcpyAsync(out->top, o.top, 4 * n, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess && out->bottom) e = hipMemcpyAsync(out->bottom, o.bottom, 4 * n, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess && out->intensity) e = hipMemcpyAsync(out->intensity, o.intensity, n, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess && out->n_voxels) e = hipMemcpyAsync(out->n_voxels, o.n_voxels, 4 * n, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess && out->n_points) e = hipMemcpyAsync(out->n_points, o.n_points, 8 * n, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(c, d, sizeof(c), hipMemcpyDeviceToHost, ctx->stream);
        return e;
      });
  if (rc) return rc;
  if (counts) for (int i = 0; i < 5; ++i) counts[i] = c[i];
  return SVO_OK;
}

// ----------------------------------------------------------------------------- removal and move
static int voxel_remove_launch(svo_voxel_map* m, const svo_cloud_point* points, int n, const double* m12, uint64_t* counts) {
  svo_ctx* ctx = m->ctx;
  VoxelRemoveArgs a{};
  a.pts = points; a.n = n; a.t = m->t;
  memcpy(a.m, m12, sizeof(a.m));
  a.voxel_size = m->prm.voxel_size; a.max_depth = m->prm.max_depth;
  a.counts = reinterpret_cast<u64*>(counts);
  if (counts) SVO_HIP_CHECK(ctx, hipMemsetAsync(counts, 0, 4 * sizeof(u64), ctx->stream));
  hipLaunchKernelGGL(voxel_remove_kernel, dim3((unsigned)voxel_record_groups(n)), dim3(VX_T), 0, ctx->stream, a);
  SVO_HIP_CHECK(ctx, hipGetLastError());
  return SVO_OK;
}

extern "C" int svo_voxel_map_remove_dev(svo_voxel_map* m, const svo_cloud_point* points, int n, const double* m12, uint64_t* counts) {
  if (!m) return SVO_ERR_INVALID;
  svo_ctx* ctx = m->ctx;
  svo_use_device(ctx);
  SVO_ARGS_CHECK(ctx, voxel_cloud_check(points, n, m12, VOXEL_REMOVE_TEXTS, &err));
  SVO_ARGS_CHECK(ctx, voxel_counts_check(counts, VOXEL_REMOVE_TEXTS, &err));
  if (n == 0) return SVO_OK;
  SvoProfScope prof(ctx, SVO_PROF_VOXEL_REMOVE);
  return voxel_remove_launch(m, points, n, m12, counts);
}

extern "C" int svo_voxel_map_remove_pose7_dev(svo_voxel_map* m, const svo_cloud_point* points, int n, const double* pose7, uint64_t* counts) {
  double m12[12];
  const int rc = voxel_pose7(m, pose7, voxel_pose7_to_cam_to_world, m12, "voxel_map_remove_pose7: null pose7");
  return rc ? rc : svo_voxel_map_remove_dev(m, points, n, m12, counts);
}

extern "C" int svo_voxel_map_remove_sync(svo_voxel_map* m, const svo_cloud_point* points, int n, const double* m12, uint64_t* counts) {
  if (!m) return SVO_ERR_INVALID;
  svo_ctx* ctx = m->ctx;
  svo_use_device(ctx);
  SVO_REQUIRE(ctx, counts, "voxel_map_remove_sync: null counts");
  u64 c[4] = {0, 0, 0, 0};
  SvoScratch scratch(ctx);
  u64* d = scratch.take<u64>(4);  // the context's scratch: this call ends with the stream drained
  SVO_REQUIRE(ctx, d, "voxel_map_remove_sync: the context has no scratch");
  const int rc = svo_host_call(
      ctx, "voxel_map_remove_sync", hipSuccess, [&] { return svo_voxel_map_remove_dev(m, points, n, m12, reinterpret_cast<uint64_t*>(d)); },
      [&] { return n > 0 ? hipMemcpyAsync(c, d, sizeof(c), hipMemcpyDeviceToHost, ctx->stream) : hipSuccess; });
  if (rc) return rc;
  for (int i = 0; i < 4; ++i) counts[i] = c[i];
  return SVO_OK;
}

extern "C" int svo_voxel_map_move_dev(svo_voxel_map* m, const svo_cloud_point* points, int n, const double* from_m12, const double* to_m12,
                                      uint64_t* counts) {
  if (!m) return SVO_ERR_INVALID;
  svo_ctx* ctx = m->ctx;
  svo_use_device(ctx);
  SVO_ARGS_CHECK(ctx, voxel_cloud_check(points, n, from_m12, VOXEL_MOVE_TEXTS, &err));
  SVO_REQUIRE(ctx, to_m12, "voxel_map_move: null to_m12");
  SVO_ARGS_CHECK(ctx, voxel_counts_check(counts, VOXEL_MOVE_TEXTS, &err));
  if (n == 0) return SVO_OK;
  if (memcmp(from_m12, to_m12, 12 * sizeof(double)) == 0) return SVO_OK;  // the same bits: the cloud is where it belongs
  SvoProfScope prof(ctx, SVO_PROF_VOXEL_MOVE);
  const int rc = voxel_remove_launch(m, points, n, from_m12, counts);
  return rc ? rc : voxel_insert_launch(m, points, n, to_m12);
}

extern "C" int svo_voxel_map_move_pose7_dev(svo_voxel_map* m, const svo_cloud_point* points, int n, const double* from_pose7,
                                            const double* to_pose7, uint64_t* counts) {
  double from[12], to[12];
  int rc = voxel_pose7(m, from_pose7, voxel_pose7_to_cam_to_world, from, "voxel_map_move_pose7: null from_pose7");
  if (!rc) rc = voxel_pose7(m, to_pose7, voxel_pose7_to_cam_to_world, to, "voxel_map_move_pose7: null to_pose7");
  return rc ? rc : svo_voxel_map_move_dev(m, points, n, from, to, counts);
}

// ----------------------------------------------------------------------------- the keyframe ledger
// The bookkeeping is host/voxel_ledger.h; here are the device copy of the held clouds and the calls.
struct svo_voxel_ledger {
  svo_voxel_map* map = nullptr;
  VoxelLedgerTable table;
  svo_cloud_point* d_points = nullptr;  // max_keyframes slots of max_points records
  svo_cloud_point* at(int slot) const { return d_points + (size_t)slot * (size_t)table.max_points(); }
};

extern "C" int svo_voxel_ledger_bytes(const svo_voxel_ledger_params* params, size_t* bytes) { return VoxelLedgerTable::bytes(params, bytes); }

extern "C" int svo_voxel_ledger_create(svo_voxel_map* map, const svo_voxel_ledger_params* params, svo_voxel_ledger** out) {
  if (!map) return SVO_ERR_INVALID;
  svo_ctx* ctx = map->ctx;
  svo_use_device(ctx);
  SVO_REQUIRE(ctx, out, "voxel_ledger_create: null out");
  *out = nullptr;
  svo_voxel_ledger* l = new svo_voxel_ledger();
  l->map = map;
  const char* err = nullptr;
  if (l->table.init(params, &err)) { ctx->err = err; delete l; return SVO_ERR_INVALID; }
  size_t bytes = 0;
  VoxelLedgerTable::bytes(params, &bytes);
  const hipError_t e = hipMalloc((void**)&l->d_points, bytes);
  if (e != hipSuccess) {
    ctx->err = std::string("voxel_ledger_create: hipMalloc of the held clouds: ") + hipGetErrorString(e);
    delete l;
    return SVO_ERR_HIP;
  }
  *out = l;
  return SVO_OK;
}

extern "C" void svo_voxel_ledger_destroy(svo_voxel_ledger* l) {
  if (!l) return;
  svo_use_device(l->map->ctx);
  (void)hipStreamSynchronize(l->map->ctx->stream);
  (void)hipFree(l->d_points);
  delete l;
}

extern "C" int svo_voxel_ledger_insert_pose7_dev(svo_voxel_ledger* l, int64_t id, const svo_cloud_point* points, int n, const double* pose7) {
  if (!l) return SVO_ERR_INVALID;
  svo_voxel_map* m = l->map;
  svo_ctx* ctx = m->ctx;
  svo_use_device(ctx);
  SVO_REQUIRE(ctx, pose7, "voxel_ledger_insert: null pose7");
  SVO_REQUIRE(ctx, points || n <= 0, "voxel_ledger_insert: null points");
  SVO_REQUIRE(ctx, ((uintptr_t)points & 3u) == 0, "voxel_ledger_insert: points must be 4-byte aligned");
  const char* err = nullptr;
  int slot = -1;
  if (l->table.admit(id, n, &slot, &err)) { ctx->err = err; return SVO_ERR_INVALID; }
  double m12[12];
  voxel_pose7_to_cam_to_world(pose7, m12);
  if (n > 0) {  // the ledger's own copy first: the caller's cloud is valid only until its next process call
    SVO_HIP_CHECK(ctx, hipMemcpyAsync(l->at(slot), points, sizeof(svo_cloud_point) * (size_t)n, hipMemcpyDeviceToDevice, ctx->stream));
    SvoProfScope prof(ctx, SVO_PROF_VOXEL_INSERT);
    const int rc = voxel_insert_launch(m, l->at(slot), n, m12);
    if (rc) return rc;
  }
  l->table.hold(slot, id, n, pose7, m12);
  return SVO_OK;
}

extern "C" int svo_voxel_ledger_update_pose7(svo_voxel_ledger* l, int64_t id, const double* pose7, uint64_t* counts) {
  if (!l) return SVO_ERR_INVALID;
  svo_ctx* ctx = l->map->ctx;
  svo_use_device(ctx);
  SVO_REQUIRE(ctx, pose7, "voxel_ledger_update: null pose7");
  const char* err = nullptr;
  int slot = -1;
  if (l->table.find(id, &slot, "voxel_ledger_update: unknown id", &err)) { ctx->err = err; return SVO_ERR_INVALID; }
  double m12[12];
  voxel_pose7_to_cam_to_world(pose7, m12);
  const VoxelLedgerSlot& s = l->table.slot(slot);
  const int rc = svo_voxel_map_move_dev(l->map, l->at(slot), s.n, s.m12, m12, counts);
  if (rc) return rc;
  l->table.moved(slot, pose7, m12);
  return SVO_OK;
}

extern "C" int svo_voxel_ledger_retire(svo_voxel_ledger* l, int64_t id) {
  if (!l) return SVO_ERR_INVALID;
  svo_ctx* ctx = l->map->ctx;
  const char* err = nullptr;
  int slot = -1;
  if (l->table.find(id, &slot, "voxel_ledger_retire: unknown id", &err)) { ctx->err = err; return SVO_ERR_INVALID; }
  l->table.release(slot);  // the next copy into the slot is behind every launch that read it: one stream
  return SVO_OK;
}

extern "C" int svo_voxel_ledger_remove(svo_voxel_ledger* l, int64_t id, uint64_t* counts) {
  if (!l) return SVO_ERR_INVALID;
  svo_ctx* ctx = l->map->ctx;
  svo_use_device(ctx);
  const char* err = nullptr;
  int slot = -1;
  if (l->table.find(id, &slot, "voxel_ledger_remove: unknown id", &err)) { ctx->err = err; return SVO_ERR_INVALID; }
  const VoxelLedgerSlot& s = l->table.slot(slot);
  const int rc = svo_voxel_map_remove_dev(l->map, l->at(slot), s.n, s.m12, counts);
  if (rc) return rc;
  l->table.release(slot);
  return SVO_OK;
}

extern "C" int svo_voxel_ledger_ids(svo_voxel_ledger* l, int64_t* ids, int capacity, int* n) {
  if (!l) return SVO_ERR_INVALID;
  const char* err = nullptr;
  if (l->table.ids(ids, capacity, n, &err)) { l->map->ctx->err = err; return SVO_ERR_INVALID; }
  return SVO_OK;
}

extern "C" int svo_voxel_ledger_get(svo_voxel_ledger* l, int64_t id, double* pose7, int* n, const svo_cloud_point** points) {
  if (!l) return SVO_ERR_INVALID;
  const char* err = nullptr;
  int slot = -1;
  if (l->table.find(id, &slot, "voxel_ledger_get: unknown id", &err)) { l->map->ctx->err = err; return SVO_ERR_INVALID; }
  const VoxelLedgerSlot& s = l->table.slot(slot);
  if (pose7) memcpy(pose7, s.pose7, sizeof(s.pose7));
  if (n) *n = s.n;
  if (points) *points = l->at(slot);
  return SVO_OK;
}
