// The voxel map sight lines' logic that needs no GPU (include/svo.h, "Voxel map sight lines"): the argument checks with
// their message texts and their order, the sizes, the defaults, and - as __host__ __device__ inline code, so that the kernels and
// a CPU program run the same statements - a ray's set-up, the plain walk, the block-skipping walk, a record's result and a
// pixel's disparity.  Integer work apart from the few ordered f64 operations of the set-up and of the result (+ - * / floor sqrt,
// no contraction).  A refusal is SVO_ERR_INVALID with *err set to the message; csrc/voxel_rays.hip stores it in the context and
// keeps no second copy of anything here.  tests/sanitize/voxel_rays_args_test.cpp walks all of it on a CPU.
#ifndef SVO_VOXEL_RAYS_H_
#define SVO_VOXEL_RAYS_H_
#include "voxel_locate.h"

constexpr int VOXEL_RAYS_MAX = 1 << 20;        // rays per call
constexpr int VOXEL_RAYS_THREADS = 256;        // one ray per lane; four 8 x 8 pixel tiles per workgroup of the camera form
constexpr int VOXEL_COARSE_THREADS = 256;      // one fine word per thread
constexpr int VOXEL_RAYS_COUNTS = 6, VOXEL_RAYCAST_COUNTS = 7;
constexpr uint32_t VOXEL_RAY_NO_CELL = 0xFFFFFFFFu;
constexpr long long VOXEL_RAY_STILL = 1ll << 62;  // the X of an axis the ray does not move along
// svo_voxel_map_raycast hands the coarse volume to the walk: on the camera form the block-skipping walk is faster by 35 to 38 % at
// 0.05 m voxels, by 20 to 24 % at the map's default 0.1 m, and level with the plain one at 0.2 m.  With the coarse
// launch counted, a single view gains 27 to 29 %, 10 to 14 % and loses 1 to 21 % at the three sizes.
constexpr bool VOXEL_RAYCAST_HOST_SKIPS = true;

// ----------------------------------------------------------------------------- sizes
inline size_t voxel_coarse_words(const int* dims) {  // dims are checked
  return ((size_t)((dims[0] + 7) >> 3) * (size_t)((dims[1] + 7) >> 3) * (size_t)((dims[2] + 7) >> 3) + 63) >> 6;
}

inline int voxel_coarse_bytes(const int* dims, size_t* bytes) {
  if (!bytes) return SVO_ERR_INVALID;
  *bytes = 0;
  const char* err = nullptr;
  if (voxel_occupancy_dims_check(dims, &err)) return SVO_ERR_INVALID;
  *bytes = 8 * voxel_coarse_words(dims);
  return SVO_OK;
}

inline int voxel_raycast_default_params(svo_voxel_raycast_params* p) {
  if (!p) return SVO_ERR_INVALID;
  p->max_range = 30.0f; p->min_step = 1;
  return SVO_OK;
}

// ----------------------------------------------------------------------------- the checks, in the contract's order
inline int voxel_coarse_check(const void* bits, const int* dims, const void* coarse, const char** err) {
  if (const int rc = voxel_occupancy_dims_check(dims, err)) return rc;
  if (const int rc = voxel_occupancy_bits_check(bits, err)) return rc;
  VOXEL_REFUSE(coarse, "voxel_occupancy_coarse: null coarse");
  VOXEL_REFUSE(((uintptr_t)coarse & 7u) == 0, "voxel_occupancy_coarse: coarse must be 8-byte aligned");
  return SVO_OK;
}

// Items 5 to 7 of the rays' refusals, which the camera form shares.
inline int voxel_rays_volume_check(const void* bits, const void* coarse, const int* origin, const int* dims, const char** err) {
  if (const int rc = voxel_occupancy_origin_check(origin, err)) return rc;
  if (const int rc = voxel_occupancy_dims_check(dims, err)) return rc;
  if (const int rc = voxel_occupancy_bits_check(bits, err)) return rc;
  VOXEL_REFUSE(((uintptr_t)coarse & 7u) == 0, "voxel_occupancy_rays: coarse must be 8-byte aligned");
  return SVO_OK;
}

// device: the _dev entry's pointers, whose alignment the kernel relies on; the host form's arrays may have any alignment and its
// counts may be null.
inline int voxel_rays_check(const void* bits, const void* coarse, const int* origin, const int* dims, const void* rays, int n, int min_step,
                            const void* hits, const void* counts, bool device, const char** err) {
  VOXEL_REFUSE(n >= 0, "voxel_occupancy_rays: n must not be negative");
  VOXEL_REFUSE(n <= VOXEL_RAYS_MAX, "voxel_occupancy_rays: n beyond 2^20");
  VOXEL_REFUSE(min_step >= 0 && min_step <= 255, "voxel_occupancy_rays: min_step outside 0..255");
  if (const int rc = voxel_rays_volume_check(bits, coarse, origin, dims, err)) return rc;
  VOXEL_REFUSE(hits, "voxel_occupancy_rays: null hits");
  if (device) {
    VOXEL_REFUSE(((uintptr_t)hits & 15u) == 0, "voxel_occupancy_rays: hits must be 16-byte aligned");
    VOXEL_REFUSE(((uintptr_t)counts & 7u) == 0, "voxel_occupancy_rays: counts must be 8-byte aligned");
  }
  if (n == 0) return SVO_OK;
  VOXEL_REFUSE(rays, "voxel_occupancy_rays: null rays");
  if (device) VOXEL_REFUSE(((uintptr_t)rays & 15u) == 0, "voxel_occupancy_rays: rays must be 16-byte aligned");
  return SVO_OK;
}

inline int voxel_raycast_params_check(int width, int height, const svo_camera_info* cam, const double* c2w12, const svo_voxel_raycast_params* prm,
                                      int max_width, int max_height, const char** err) {
  VOXEL_REFUSE(cam, "voxel_occupancy_raycast: null cam");
  VOXEL_REFUSE(c2w12, "voxel_occupancy_raycast: null c2w12");
  VOXEL_REFUSE(prm, "voxel_occupancy_raycast: null params");
  VOXEL_REFUSE(prm->max_range >= 0.0f && prm->max_range <= FLT_MAX, "voxel_occupancy_raycast: max_range must be finite and not negative");  // a NaN fails
  VOXEL_REFUSE(prm->min_step >= 0 && prm->min_step <= 255, "voxel_occupancy_raycast: min_step outside 0..255");
  VOXEL_REFUSE(width >= 1 && width <= max_width, "voxel_occupancy_raycast: width below 1 or beyond the context's limit");
  VOXEL_REFUSE(height >= 1 && height <= max_height, "voxel_occupancy_raycast: height below 1 or beyond the context's limit");
  VOXEL_REFUSE(cam->focal > 0.0 && cam->focal <= DBL_MAX, "voxel_occupancy_raycast: focal must be finite and > 0");
  VOXEL_REFUSE(cam->baseline > 0.0 && cam->baseline <= DBL_MAX, "voxel_occupancy_raycast: baseline must be finite and > 0");
  return SVO_OK;
}

inline int voxel_raycast_check(const void* bits, const void* coarse, const int* origin, const int* dims, int width, int height, const svo_camera_info* cam,
                               const double* c2w12, const svo_voxel_raycast_params* prm, int max_width, int max_height, const void* disp16,
                               const void* cell, const void* counts, const char** err) {
  if (const int rc = voxel_raycast_params_check(width, height, cam, c2w12, prm, max_width, max_height, err)) return rc;
  if (const int rc = voxel_rays_volume_check(bits, coarse, origin, dims, err)) return rc;
  VOXEL_REFUSE(disp16, "voxel_occupancy_raycast: null disp16");
  VOXEL_REFUSE(((uintptr_t)disp16 & 1u) == 0, "voxel_occupancy_raycast: disp16 must be 2-byte aligned");
  VOXEL_REFUSE(((uintptr_t)cell & 3u) == 0, "voxel_occupancy_raycast: cell must be 4-byte aligned");
  VOXEL_REFUSE(((uintptr_t)counts & 7u) == 0, "voxel_occupancy_raycast: counts must be 8-byte aligned");
  return SVO_OK;
}

// The host convenience's own arguments, before the volume's origin is formed.
inline int voxel_map_raycast_check(int min_count, const int* dims, int width, int height, const svo_camera_info* cam, const double* c2w12,
                                   const svo_voxel_raycast_params* prm, int max_width, int max_height, const void* disp16, const char** err) {
  VOXEL_REFUSE(min_count >= 1, "voxel_map_raycast: min_count must be at least 1");
  if (const int rc = voxel_raycast_params_check(width, height, cam, c2w12, prm, max_width, max_height, err)) return rc;
  if (const int rc = voxel_occupancy_dims_check(dims, err)) return rc;
  VOXEL_REFUSE(disp16, "voxel_map_raycast: null disp16");
  return SVO_OK;
}

// ----------------------------------------------------------------------------- item 2: a ray's set-up
struct VoxelRaySetup {
  long long p[3], L[3];
  int D[3];
  double rootS, m;
};

// o, d, max_range already doubles (a record's floats widened, a pixel's doubles as they are); false: REJECTED.
VOXEL_HD inline bool voxel_ray_setup(const double* o, const double* d, double max_range, float voxel_size, const int* origin, VoxelRaySetup* s) {
  bool fin = max_range >= -DBL_MAX && max_range <= DBL_MAX;
  for (int r = 0; r < 3; ++r) fin = fin && o[r] >= -DBL_MAX && o[r] <= DBL_MAX && d[r] >= -DBL_MAX && d[r] <= DBL_MAX;  // a NaN fails
  if (!fin || max_range < 0.0) return false;
  double m = fabs(d[0]);
  m = fabs(d[1]) > m ? fabs(d[1]) : m;
  m = fabs(d[2]) > m ? fabs(d[2]) : m;
  if (m == 0.0) return false;
  const double vs = (double)voxel_size;
  double q[3];
  for (int r = 0; r < 3; ++r) {
    q[r] = o[r] / vs;
    if (!(q[r] >= -VOXEL_LOCATE_LIMIT && q[r] < VOXEL_LOCATE_LIMIT)) return false;
  }
  long long S = 0;
  for (int r = 0; r < 3; ++r) {
    s->p[r] = (long long)floor(q[r] * 256.0) - 256ll * (long long)origin[r];
    s->D[r] = (int)floor((d[r] / m) * 16384.0 + 0.5);
    S += (long long)s->D[r] * (long long)s->D[r];
  }
  s->rootS = sqrt((double)S);
  s->m = m;
  const double R = (max_range / vs) * 256.0;
  for (int r = 0; r < 3; ++r) {
    const double l = floor((R * (double)(s->D[r] < 0 ? -s->D[r] : s->D[r])) / s->rootS);
    s->L[r] = (long long)(l < 1099511627776.0 ? l : 1099511627776.0);  // 2^40; R is finite: no NaN
  }
  return true;
}

VOXEL_HD inline bool voxel_ray_setup_record(const svo_voxel_ray& ray, float voxel_size, const int* origin, VoxelRaySetup* s) {
  const double o[3] = {(double)ray.ox, (double)ray.oy, (double)ray.oz}, d[3] = {(double)ray.dx, (double)ray.dy, (double)ray.dz};
  return voxel_ray_setup(o, d, (double)ray.max_range, voxel_size, origin, s);
}

// A pixel's ray: item 8.
VOXEL_HD inline void voxel_pixel_ray(const double* m12, double focal, double cx, double cy, int x, int y, double* o, double* d) {
  const double v0 = ((double)x - cx) / focal, v1 = ((double)y - cy) / focal;
  for (int r = 0; r < 3; ++r) {
    d[r] = m12[4 * r] * v0 + m12[4 * r + 1] * v1 + m12[4 * r + 2];
    o[r] = m12[4 * r + 3];
  }
}

// ----------------------------------------------------------------------------- item 3: the walk
enum { VOXEL_RAY_HIT = 0, VOXEL_RAY_LEFT = 1, VOXEL_RAY_RANGE = 2, VOXEL_RAY_OUTSIDE = 3, VOXEL_RAY_REJECTED = 4 };

struct VoxelRayEnd {
  int code, axis;  // axis: the a of the last crossing considered, 3 where there was none
  uint32_t cell, steps;
  long long n;      // that crossing's n_a
  int absD;         // and its |D_a|
};

VOXEL_HD inline VoxelRayEnd voxel_ray_no_walk(int code) { return VoxelRayEnd{code, 3, VOXEL_RAY_NO_CELL, 0u, 0ll, 1}; }

// The bit of cell c; B < 2^30.
VOXEL_HD inline uint32_t voxel_ray_cell(const int* c, const int* dims) {
  return (uint32_t)c[0] + (uint32_t)dims[0] * ((uint32_t)c[1] + (uint32_t)dims[1] * (uint32_t)c[2]);
}

// v[a] and v[a] += x for a run-time a in 0..2, by selects: an array indexed by a run-time value would live in scratch memory.
template <typename T>
VOXEL_HD inline T voxel_ray_pick(const T* v, int a) { return a == 0 ? v[0] : (a == 1 ? v[1] : v[2]); }
template <typename T>
VOXEL_HD inline void voxel_ray_add(T* v, int a, T x) {
  v[0] += a == 0 ? x : (T)0;
  v[1] += a == 1 ? x : (T)0;
  v[2] += a == 2 ? x : (T)0;
}

// SKIP: the block-skipping form, which reads `coarse` (item 1's output for `bits`); the same values either way.
template <bool SKIP>
VOXEL_HD inline VoxelRayEnd voxel_ray_walk(const VoxelRaySetup& s, const int* dims, const uint64_t* bits, const uint64_t* coarse, int min_step) {
  int c[3], dir[3], aD[3];
  long long n[3], X[3], w256[3];
  for (int r = 0; r < 3; ++r) {
    c[r] = (int)(s.p[r] >> 8);
    if (c[r] < 0 || c[r] >= dims[r]) return voxel_ray_no_walk(VOXEL_RAY_OUTSIDE);
  }
  for (int r = 0; r < 3; ++r) {
    const int D = s.D[r], f = (int)(s.p[r] & 255);
    dir[r] = D > 0 ? 1 : (D < 0 ? -1 : 0);
    aD[r] = D < 0 ? -D : D;
    n[r] = D > 0 ? 256 - f : f;
  }
  for (int r = 0; r < 3; ++r) {
    const int a1 = aD[(r + 1) % 3], a2 = aD[(r + 2) % 3];
    const long long w = (long long)(a1 > 1 ? a1 : 1) * (long long)(a2 > 1 ? a2 : 1);
    w256[r] = 256 * w;
    X[r] = dir[r] ? n[r] * w : VOXEL_RAY_STILL;
  }
  const int cd0 = (dims[0] + 7) >> 3, cd1 = (dims[1] + 7) >> 3;
  VoxelRayEnd e{VOXEL_RAY_HIT, 3, voxel_ray_cell(c, dims), 0u, 0ll, 1};
  unsigned k = 0;
  if (min_step == 0 && (bits[e.cell >> 6] >> (e.cell & 63) & 1ull)) return e;
  const int cap = dims[0] + dims[1] + dims[2];  // no walk is longer; the explicit bound of the loop
  for (int it = 0; it < cap; ++it) {
    if (SKIP) {
      const uint32_t Bc = (uint32_t)(c[0] >> 3) + (uint32_t)cd0 * ((uint32_t)(c[1] >> 3) + (uint32_t)cd1 * (uint32_t)(c[2] >> 3));
      if (!(coarse[Bc >> 6] >> (Bc & 63) & 1ull)) {
        // the crossings that leave this 8-block (or the volume through it), per moving axis; then the first of them
        int ex[3];
        long long Xe[3];
        for (int r = 0; r < 3; ++r) {
          const int up = 8 - (c[r] & 7), room = dims[r] - c[r];
          ex[r] = dir[r] > 0 ? (up < room ? up : room) : (c[r] & 7) + 1;
          Xe[r] = dir[r] ? X[r] + w256[r] * (long long)(ex[r] - 1) : VOXEL_RAY_STILL;
        }
        int a = Xe[1] < Xe[0] ? 1 : 0;
        long long Xa = Xe[1] < Xe[0] ? Xe[1] : Xe[0];
        if (Xe[2] < Xa) { a = 2; Xa = Xe[2]; }
        int ms[3];
        bool ok = true;
        for (int r = 0; r < 3; ++r) {
          int cnt = 0;
          if (r == a) {
            cnt = ex[r] - 1;
          } else if (dir[r]) {
            long long x = X[r];
            for (int i = 0; i < 7; ++i) {
              cnt += (r < a ? x <= Xa : x < Xa) ? 1 : 0;
              x += w256[r];
            }
          }
          ms[r] = cnt;
          ok = ok && (cnt == 0 || n[r] + 256ll * (long long)(cnt - 1) <= s.L[r]);
        }
        if (ok) {
          for (int r = 0; r < 3; ++r) {
            c[r] += dir[r] * ms[r];
            n[r] += 256ll * (long long)ms[r];
            X[r] += w256[r] * (long long)ms[r];  // a still axis has ms 0
            k += (unsigned)ms[r];
          }
          e.cell = voxel_ray_cell(c, dims);
        }
      }
    }
    int a = X[1] < X[0] ? 1 : 0;
    if (X[2] < (a ? X[1] : X[0])) a = 2;
    e.axis = a; e.n = voxel_ray_pick(n, a); e.absD = voxel_ray_pick(aD, a); e.steps = k;
    if (e.n > voxel_ray_pick(s.L, a)) { e.code = VOXEL_RAY_RANGE; return e; }
    voxel_ray_add(c, a, voxel_ray_pick(dir, a));
    const int ca = voxel_ray_pick(c, a);
    if (ca < 0 || ca >= voxel_ray_pick(dims, a)) { e.code = VOXEL_RAY_LEFT; return e; }
    ++k;
    e.cell = voxel_ray_cell(c, dims);
    e.steps = k;
    if (k >= (unsigned)min_step && (bits[e.cell >> 6] >> (e.cell & 63) & 1ull)) return e;
    voxel_ray_add(n, a, 256ll);
    voxel_ray_add(X, a, voxel_ray_pick(w256, a));
  }
  e.code = VOXEL_RAY_LEFT;  // not reached: the cap is the walk's own bound
  return e;
}

// ----------------------------------------------------------------------------- item 4: the record
VOXEL_HD inline svo_voxel_ray_hit voxel_ray_result(const VoxelRayEnd& e, const VoxelRaySetup& s, float voxel_size) {
  svo_voxel_ray_hit h;
  h.cell = e.cell;
  h.steps = e.steps;
  h.dist = e.axis == 3 ? 0.0f : (float)((((double)e.n * s.rootS) / (double)e.absD) / 256.0 * (double)voxel_size);
  h.status = (uint32_t)e.code | (uint32_t)e.axis << 8;
  return h;
}

// Item 8: the pixel's value in sixteenths, or FILTERED (-16).
VOXEL_HD inline int voxel_ray_disp16(const VoxelRayEnd& e, const VoxelRaySetup& s, float voxel_size, double focal, double baseline) {
  if (e.code != VOXEL_RAY_HIT || e.steps < 1u) return -16;
  const double z = ((double)e.n * (double)voxel_size * 64.0) / ((double)e.absD * s.m);
  const double d16 = floor((focal * baseline) / z * 16.0 + 0.5);
  return 1.0 <= d16 && d16 <= 32767.0 ? (int)d16 : -16;  // a crossing at n = 0 gives infinity, which fails
}

// ----------------------------------------------------------------------------- launch geometry
inline size_t voxel_coarse_groups(const int* dims) { return voxel_div_up(voxel_occupancy_words(dims), VOXEL_COARSE_THREADS); }
inline size_t voxel_rays_groups(int n) { return voxel_div_up((size_t)n, VOXEL_RAYS_THREADS); }
inline size_t voxel_raycast_tiles_x(int width) { return ((size_t)width + 7) >> 3; }
inline size_t voxel_raycast_groups(int width, int height) {  // 8 x 8 pixel tiles, one per wavefront
  return voxel_div_up(voxel_raycast_tiles_x(width) * (((size_t)height + 7) >> 3), VOXEL_RAYS_THREADS / 64);
}

#endif  // SVO_VOXEL_RAYS_H_
