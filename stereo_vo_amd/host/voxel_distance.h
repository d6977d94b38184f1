// The voxel map distance field's logic that needs no GPU (include/svo.h, "Voxel map distance field"): the argument
// checks with their message texts and their order, the sizes, R2, the defaults, the launch geometry, and - as __host__ __device__
// inline code, so that the kernels and a CPU program run the same statements - the axis-0 search of a row's words, the outward
// search along axis 1 or 2, a cell's clearance and a sphere's record.  Integer work apart from the clearance's f64 root and product
// and the few ordered f64 operations of a sphere (no contraction).  A refusal is SVO_ERR_INVALID with *err set to the message;
// csrc/voxel_distance.hip stores it in the context and keeps no second copy of anything here.
// tests/sanitize/voxel_distance_args_test.cpp walks all of it on a CPU.
#ifndef SVO_VOXEL_DISTANCE_H_
#define SVO_VOXEL_DISTANCE_H_
#include "voxel_locate.h"

constexpr int VOXEL_DISTANCE_THREADS = 256;   // one cell per lane, lanes along axis 0: four words of the volume per workgroup
constexpr int VOXEL_DISTANCE_MAX = 254;       // max_dist: 254^2 = 64,516 fits the u16 beside NONE16
constexpr int VOXEL_DISTANCE_STEPS = 4;       // outward steps whose loads are in flight together (§7k's CL_STEPS)
constexpr int VOXEL_DISTANCE_COUNTS = 4, VOXEL_DISTANCE_QUERY_COUNTS = 6;
constexpr int VOXEL_DISTANCE_QUERY_MAX = 1 << 20;  // spheres per call
constexpr uint16_t VOXEL_DISTANCE_NONE16 = 0xFFFFu;
constexpr uint32_t VOXEL_DISTANCE_NONE = 0xFFFFFFFFu;
constexpr int VOXEL_DISTANCE_NO_OFFSET = 0x7FFF;   // the axis-0 pass found no source within max_dist
enum { VOXEL_SPHERE_FREE = 0, VOXEL_SPHERE_COLLIDES = 1, VOXEL_SPHERE_OUTSIDE = 2, VOXEL_SPHERE_REJECTED = 3 };

// ----------------------------------------------------------------------------- sizes, defaults, R2
inline size_t voxel_distance_cells(const int* dims) { return (size_t)dims[0] * (size_t)dims[1] * (size_t)dims[2]; }  // dims are checked

// What passes between the three launches, in the caller's workspace (rule 7).  Without `nearest`: a u8 |offset| per cell from the
// axis-0 pass (255: none), then a u16 partial square from the axis-1 pass: 3 bytes per cell.  With it: an i16 signed offset, then
// a u32 that packs both offsets (9 bits each, biased by 256): 6 bytes per cell.  The second part starts at a multiple of 64 bytes.
struct VoxelDistanceLayout {
  size_t second, total;  // byte offset of the axis-1 pass's output; bytes in all
};
inline VoxelDistanceLayout voxel_distance_layout(const int* dims, bool nearest) {
  const size_t n = voxel_distance_cells(dims);
  return nearest ? VoxelDistanceLayout{2 * n, 6 * n} : VoxelDistanceLayout{n, 3 * n};
}

inline int voxel_distance_workspace_bytes(const int* dims, int want_nearest, size_t* bytes) {
  if (!bytes) return SVO_ERR_INVALID;
  *bytes = 0;
  const char* err = nullptr;
  if (voxel_occupancy_dims_check(dims, &err)) return SVO_ERR_INVALID;
  *bytes = voxel_distance_layout(dims, want_nearest != 0).total;
  return SVO_OK;
}

inline int voxel_distance_bytes(const int* dims, size_t* bytes) {
  if (!bytes) return SVO_ERR_INVALID;
  *bytes = 0;
  const char* err = nullptr;
  if (voxel_occupancy_dims_check(dims, &err)) return SVO_ERR_INVALID;
  *bytes = 2 * voxel_distance_cells(dims);
  return SVO_OK;
}

// 32 voxels, no inflation.  NOT tuned on real data.  The voxel size is taken for the day the defaults depend on it.
inline int voxel_distance_default_params(float voxel_size, svo_voxel_distance_params* p) {
  if (!p || !(voxel_size > 0.0f && voxel_size <= FLT_MAX)) return SVO_ERR_INVALID;
  p->max_dist = 32; p->inflate_radius = 0.0f;
  return SVO_OK;
}

// Rule 4's R2 = floor(rc * rc) clamped to max_dist^2, rc = inflate_radius / voxel_size in f64: §7k's clearance_r2.  The arguments
// have passed the checks, so nothing is a NaN; a quotient or a square that overflows is +infinity and takes the clamp.
inline uint32_t voxel_distance_r2(float inflate_radius, float voxel_size, int max_dist) {
  const double rc = (double)inflate_radius / (double)voxel_size;
  const double q = floor(rc * rc), cap = (double)max_dist * (double)max_dist;
  return (uint32_t)(q < cap ? q : cap);
}

// ----------------------------------------------------------------------------- the checks, in the contract's order
inline int voxel_distance_params_check(const svo_voxel_distance_params* p, const char** err) {
  VOXEL_REFUSE(p, "voxel_occupancy_distance: null params");
  VOXEL_REFUSE(p->max_dist >= 1 && p->max_dist <= VOXEL_DISTANCE_MAX, "voxel_occupancy_distance: max_dist outside 1..254");
  VOXEL_REFUSE(p->inflate_radius >= 0.0f && p->inflate_radius <= FLT_MAX, "voxel_occupancy_distance: inflate_radius must be finite and not negative");  // a NaN fails
  return SVO_OK;
}

inline int voxel_distance_check(const void* bits, const int* dims, const svo_voxel_distance_params* p, const void* workspace, const svo_voxel_distance_out* o,
                                const void* counts, const char** err) {
  if (const int rc = voxel_distance_params_check(p, err)) return rc;
  if (const int rc = voxel_occupancy_dims_check(dims, err)) return rc;
  if (const int rc = voxel_occupancy_bits_check(bits, err)) return rc;
  VOXEL_REFUSE(workspace, "voxel_occupancy_distance: null workspace");
  VOXEL_REFUSE(((uintptr_t)workspace & 7u) == 0, "voxel_occupancy_distance: workspace must be 8-byte aligned");
  VOXEL_REFUSE(o, "voxel_occupancy_distance: null out");
  VOXEL_REFUSE(o->dist2, "voxel_occupancy_distance: null dist2");
  VOXEL_REFUSE(((uintptr_t)o->dist2 & 1u) == 0, "voxel_occupancy_distance: dist2 must be 2-byte aligned");
  VOXEL_REFUSE(((uintptr_t)o->nearest & 3u) == 0, "voxel_occupancy_distance: nearest must be 4-byte aligned");
  VOXEL_REFUSE(((uintptr_t)o->clearance & 3u) == 0, "voxel_occupancy_distance: clearance must be 4-byte aligned");
  VOXEL_REFUSE(((uintptr_t)o->inflated & 7u) == 0, "voxel_occupancy_distance: inflated must be 8-byte aligned");
  VOXEL_REFUSE(((uintptr_t)counts & 7u) == 0, "voxel_occupancy_distance: counts must be 8-byte aligned");
  return SVO_OK;
}

// The host convenience's own arguments; its outputs are host arrays of any alignment.
inline int voxel_map_distance_check(int min_count, const int* origin, const int* dims, const svo_voxel_distance_params* p, const svo_voxel_distance_out* o,
                                    const char** err) {
  VOXEL_REFUSE(min_count >= 1, "voxel_map_distance: min_count must be at least 1");
  if (const int rc = voxel_distance_params_check(p, err)) return rc;
  if (const int rc = voxel_occupancy_origin_check(origin, err)) return rc;
  if (const int rc = voxel_occupancy_dims_check(dims, err)) return rc;
  VOXEL_REFUSE(o, "voxel_map_distance: null out");
  VOXEL_REFUSE(o->dist2, "voxel_map_distance: null dist2");
  return SVO_OK;
}

// device: the _dev entry's pointers, whose alignment the kernel relies on; the host form's spheres, hits and counts may have any
// alignment.  dist2 is a device pointer in both.
inline int voxel_distance_query_check(const void* dist2, const int* origin, const int* dims, const void* spheres, int n, const void* hits, const void* counts,
                                      bool device, const char** err) {
  VOXEL_REFUSE(n >= 0, "voxel_distance_query: n must not be negative");
  VOXEL_REFUSE(n <= VOXEL_DISTANCE_QUERY_MAX, "voxel_distance_query: n beyond 2^20");
  if (const int rc = voxel_occupancy_origin_check(origin, err)) return rc;
  if (const int rc = voxel_occupancy_dims_check(dims, err)) return rc;
  VOXEL_REFUSE(dist2, "voxel_distance_query: null dist2");
  VOXEL_REFUSE(((uintptr_t)dist2 & 1u) == 0, "voxel_distance_query: dist2 must be 2-byte aligned");
  VOXEL_REFUSE(hits, "voxel_distance_query: null hits");
  if (device) {
    VOXEL_REFUSE(((uintptr_t)hits & 15u) == 0, "voxel_distance_query: hits must be 16-byte aligned");
    VOXEL_REFUSE(((uintptr_t)counts & 7u) == 0, "voxel_distance_query: counts must be 8-byte aligned");
  }
  if (n == 0) return SVO_OK;
  VOXEL_REFUSE(spheres, "voxel_distance_query: null spheres");
  if (device) VOXEL_REFUSE(((uintptr_t)spheres & 15u) == 0, "voxel_distance_query: spheres must be 16-byte aligned");
  return SVO_OK;
}

// ----------------------------------------------------------------------------- axis 0: a row's words
// The signed offset s0 - j0 of the nearest source of the row to cell j0 = 64 * x + lane, the left one of two at equal distance, or
// VOXEL_DISTANCE_NO_OFFSET beyond max_dist.  row: the row's wpr words.  Inside the cell's own word the nearest set bit at or below
// the lane comes from a mask and a count of leading zeros, the nearest at or above it from a shift and a count of trailing zeros;
// then the neighbouring words outward, each side until its first non-zero word, ceil(max_dist / 64) words or the row's end.  Every
// load and every loop condition depends on x alone, which a wavefront shares.
VOXEL_HD inline int voxel_distance_row(const uint64_t* row, int wpr, int x, int lane, int max_dist) {
  constexpr int UNSEEN = 1 << 20;
  const uint64_t w = row[x];
  const uint64_t lo = w & (~0ull >> (63 - lane)), hi = w >> lane;
  int gl = lo ? lane - (63 - __builtin_clzll(lo)) : UNSEEN;
  int gr = hi ? __builtin_ctzll(hi) : UNSEEN;
  const int K = (max_dist + 63) >> 6;
  uint64_t wl = 0, wr = 0;
  for (int k = 1; k <= K && x - k >= 0 && !wl; ++k) {
    wl = row[x - k];
    if (wl && gl == UNSEEN) gl = lane + 64 * k - (63 - __builtin_clzll(wl));
  }
  for (int k = 1; k <= K && x + k < wpr && !wr; ++k) {
    wr = row[x + k];
    if (wr && gr == UNSEEN) gr = 64 * k - lane + __builtin_ctzll(wr);
  }
  const int g = gl <= gr ? gl : gr;
  return g > max_dist ? VOXEL_DISTANCE_NO_OFFSET : (gl <= gr ? -gl : gr);
}

// ----------------------------------------------------------------------------- axes 1 and 2: the outward search of a line
// What the pass before left per cell, by form: NEAR carries where the source is, the plain form only how far.
template <bool NEAR, bool LAST> struct VoxelDistanceIn;
template <> struct VoxelDistanceIn<false, false> { typedef uint8_t T; };   // |offset along axis 0|, 255: none
template <> struct VoxelDistanceIn<true, false> { typedef int16_t T; };    // the signed offset, VOXEL_DISTANCE_NO_OFFSET: none
template <> struct VoxelDistanceIn<false, true> { typedef uint16_t T; };   // offset0^2 + offset1^2, NONE16: none
template <> struct VoxelDistanceIn<true, true> { typedef uint32_t T; };    // (offset0 + 256) | (offset1 + 256) << 9, NONE: none

VOXEL_HD inline uint32_t voxel_distance_pack(int o0, int o1) { return (uint32_t)(o0 + 256) | (uint32_t)(o1 + 256) << 9; }

struct VoxelDistanceBest {
  uint32_t d2, at, arg;  // the partial (LAST: the whole) squared distance, NONE where nothing is within max_dist; NEAR: the source's
                         // bit number and, from the axis-1 pass, its two offsets packed
};

// One line of axis 1 (LAST false) or axis 2 (LAST true).  line: the entry of the line's cell at position 0; stride: entries between
// neighbours on the line; p: this cell's position, len: the line's length; line_bit: the bit number of the line's cell at 0.
// Outward g = 0, 1, ..: the entry at p - g before the one at p + g, each candidate g^2 + its value taken under "smaller value, then
// smaller bit number" if it is <= max_dist^2; stop when g^2 > best, STRICTLY (a candidate at g^2 == best with value 0 and a smaller
// bit number still wins the tie), past max_dist, or at the line's ends.  VOXEL_DISTANCE_STEPS steps at a time: the batch's loads, at
// positions clamped into the line so that none sits under a branch, are issued before the first test, and the tests then run in
// the steps' order, which leaves every result what the step-by-step search gives (best only falls, g^2 only grows).
template <bool NEAR, bool LAST>
VOXEL_HD inline VoxelDistanceBest voxel_distance_column(const typename VoxelDistanceIn<NEAR, LAST>::T* line, size_t stride, int p, int len, int max_dist,
                                                        uint32_t line_bit, int d0) {
  typedef typename VoxelDistanceIn<NEAR, LAST>::T In;
  const uint32_t cap = (uint32_t)(max_dist * max_dist);
  const int before = p, after = len - 1 - p;
  const int ends = before > after ? before : after, reach = max_dist < ends ? max_dist : ends;
  uint32_t best = VOXEL_DISTANCE_NONE, at = VOXEL_DISTANCE_NONE, arg = VOXEL_DISTANCE_NONE;
  for (int g0 = 0; g0 <= reach && (uint32_t)(g0 * g0) <= best; g0 += VOXEL_DISTANCE_STEPS) {
    In lo[VOXEL_DISTANCE_STEPS], hi[VOXEL_DISTANCE_STEPS];
#ifdef __HIP_DEVICE_COMPILE__
#pragma unroll
#endif
    for (int k = 0; k < VOXEL_DISTANCE_STEPS; ++k) {
      const int a = p - g0 - k, b = p + g0 + k;
      lo[k] = line[(size_t)(a > 0 ? a : 0) * stride];
      hi[k] = line[(size_t)(b < len - 1 ? b : len - 1) * stride];
    }
#ifdef __HIP_DEVICE_COMPILE__
#pragma unroll
#endif
    for (int k = 0; k < VOXEL_DISTANCE_STEPS; ++k) {
      const int g = g0 + k;
      const uint32_t g2 = (uint32_t)(g * g);
      for (int side = 0; side < 2; ++side) {
        const In e = side ? hi[k] : lo[k];
        const int q = side ? p + g : p - g;
        const bool on = g <= reach && g2 <= best && (side ? g > 0 && q < len : q >= 0);
        bool some;
        uint32_t v;
        int delta = 0, o0 = 0;
        if constexpr (!LAST && !NEAR) { some = e != 255; v = (uint32_t)e * (uint32_t)e; }
        else if constexpr (!LAST) { some = (int)e != VOXEL_DISTANCE_NO_OFFSET; o0 = some ? (int)e : 0; v = (uint32_t)(o0 * o0); delta = o0; }
        else if constexpr (!NEAR) { some = e != VOXEL_DISTANCE_NONE16; v = (uint32_t)e; }
        else {
          some = (uint32_t)e != VOXEL_DISTANCE_NONE;
          o0 = some ? (int)((uint32_t)e & 511u) - 256 : 0;
          const int o1 = some ? (int)((uint32_t)e >> 9 & 511u) - 256 : 0;
          v = (uint32_t)(o0 * o0 + o1 * o1);
          delta = o0 + d0 * o1;
        }
        const uint32_t d2 = g2 + v;  // at most 3 * 254^2
        // where `on` and `some`, the source lies inside the volume: 0 <= j < 2^30
        const uint32_t j = NEAR ? (uint32_t)((long long)line_bit + (long long)q * (long long)stride + (long long)delta) : 0u;
        const bool wins = on && some && d2 <= cap && (d2 < best || (NEAR && d2 == best && j < at));
        best = wins ? d2 : best;
        if (NEAR) {
          at = wins ? j : at;
          if (!LAST) arg = wins ? voxel_distance_pack(o0, q - p) : arg;
        }
      }
    }
  }
  return VoxelDistanceBest{best, at, arg};
}

// Rule 5.
VOXEL_HD inline float voxel_distance_clearance(uint32_t d2, float voxel_size) {
  return d2 == VOXEL_DISTANCE_NONE ? __builtin_inff() : (float)(sqrt((double)d2) * (double)voxel_size);
}

// ----------------------------------------------------------------------------- a position's cell, a sphere's record
// Rule 9's cell of the world position xyz: VOXEL_SPHERE_REJECTED, VOXEL_SPHERE_OUTSIDE, or VOXEL_SPHERE_FREE with *cell = B.
VOXEL_HD inline int voxel_distance_cell_of(const float* xyz, float voxel_size, const int* origin, const int* dims, size_t* cell) {
  const double vs = (double)voxel_size;
  double q[3];
  for (int r = 0; r < 3; ++r) {
    q[r] = (double)xyz[r] / vs;
    if (!(q[r] >= -VOXEL_LOCATE_LIMIT && q[r] < VOXEL_LOCATE_LIMIT)) return VOXEL_SPHERE_REJECTED;  // NaN and the infinities fail too
  }
  int j[3];
  for (int r = 0; r < 3; ++r) {
    j[r] = (int)floor(q[r]) - origin[r];
    if (j[r] < 0 || j[r] >= dims[r]) return VOXEL_SPHERE_OUTSIDE;
  }
  *cell = (size_t)j[0] + (size_t)dims[0] * ((size_t)j[1] + (size_t)dims[1] * (size_t)j[2]);
  return VOXEL_SPHERE_FREE;
}

// s: {x, y, z, radius}.  *beyond: the centre's cell is inside the volume and its dist2 is NONE16.
VOXEL_HD inline svo_voxel_sphere_hit voxel_distance_query_one(const float* s, float voxel_size, const int* origin, const int* dims, const uint16_t* dist2,
                                                              bool* beyond) {
  svo_voxel_sphere_hit h;
  h.cell = VOXEL_DISTANCE_NONE; h.dist2 = VOXEL_DISTANCE_NONE; h.clearance = __builtin_inff(); h.code = VOXEL_SPHERE_REJECTED;
  *beyond = false;
  const double vs = (double)voxel_size, rad = (double)s[3];
  if (!(rad >= 0.0 && rad <= DBL_MAX)) return h;  // a NaN fails
  size_t B = 0;
  h.code = (uint32_t)voxel_distance_cell_of(s, voxel_size, origin, dims, &B);
  if (h.code != VOXEL_SPHERE_FREE) return h;
  const uint16_t d = dist2[B];
  *beyond = d == VOXEL_DISTANCE_NONE16;
  h.cell = (uint32_t)B;
  h.dist2 = *beyond ? VOXEL_DISTANCE_NONE : (uint32_t)d;
  h.clearance = voxel_distance_clearance(h.dist2, voxel_size);
  const double rc = rad / vs;
  h.code = (double)h.dist2 <= floor(rc * rc) ? VOXEL_SPHERE_COLLIDES : VOXEL_SPHERE_FREE;
  return h;
}

// ----------------------------------------------------------------------------- launch geometry
inline size_t voxel_distance_groups(const int* dims) { return voxel_div_up(voxel_distance_cells(dims), VOXEL_DISTANCE_THREADS); }  // every pass
inline size_t voxel_distance_query_groups(int n) { return voxel_div_up((size_t)n, VOXEL_DISTANCE_THREADS); }

#endif  // SVO_VOXEL_DISTANCE_H_
