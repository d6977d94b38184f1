// Voxel map sight lines (include/svo.h, "Voxel map sight lines"): rays walked through the dense bit volume of the
// occupancy entry.
//
//   voxel_coarse_kernel  : one thread per fine u64 word.  A word is 64 cells along axis 0, that is eight 8-blocks, whose coarse bits
//                          are neighbours inside one coarse word (cd0 is a multiple of 8): eight byte tests and at most one relaxed
//                          atomicOr.
//   voxel_rays_kernel    : one ray per lane.  The set-up and the walk are host/voxel_rays.h's, the statements a CPU program runs
//                          too: 64-bit adds and compares and one dependent load per step (two in the block-skipping form).  The
//                          record leaves as one 16-byte store.
//   voxel_raycast_kernel : the same for one pixel per lane; a wavefront takes an 8 x 8 pixel tile, so that its rays stay in
//                          neighbouring words and end after similar step counts.
// Both ray kernels exist in two forms, SKIP = false (coarse == NULL) and true.  The counts go through ballots, a wavefront sum and
// LDS: one relaxed atomicAdd per workgroup and non-zero counter.
//
// §7c's conditions: relaxed device-scope atomics only, no fence, no waiting on another workgroup, scratch 0 (the walk's arrays of
// three are indexed by unrolled loops and by selects).  Bounds: a cell's bit number is formed only from c inside the volume, a
// coarse bit only from such a c; the walk's loop carries d0 + d1 + d2 as its explicit iteration cap.
#include "kernels.h"
#include "voxel_rays.h"

namespace {
typedef unsigned long long u64;
constexpr int VR_T = VOXEL_RAYS_THREADS;
constexpr int VR_CT = VOXEL_COARSE_THREADS;

struct VoxelCoarseArgs {
  const u64* bits;
  u64* coarse;
  u64 words;
  int wpr, d1, cd0, cd1;
};

__global__ __launch_bounds__(VR_CT) void voxel_coarse_kernel(VoxelCoarseArgs a) {
  const u64 i = (u64)blockIdx.x * VR_CT + (u64)threadIdx.x;
  if (i >= a.words) return;
  const u64 w = a.bits[i];
  if (!w) return;
  unsigned mask = 0;
#pragma unroll
  for (int b = 0; b < 8; ++b) mask |= ((w >> (8 * b)) & 0xFFull) ? 1u << b : 0u;
  const unsigned row = (unsigned)(i / (u64)a.wpr), x = (unsigned)(i % (u64)a.wpr);
  const unsigned j1 = row % (unsigned)a.d1, j2 = row / (unsigned)a.d1;
  const unsigned Bc = 8u * x + (unsigned)a.cd0 * ((j1 >> 3) + (unsigned)a.cd1 * (j2 >> 3));  // a multiple of 8, below 2^21
  __hip_atomic_fetch_or(&a.coarse[Bc >> 6], (u64)mask << (Bc & 63u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// code: 0..4, or -1 for a lane without a ray.  Every thread of the workgroup calls it.
__device__ __forceinline__ void vr_count(u64* counts, int words, int code, unsigned steps, bool kept) {
  if (!counts) return;  // uniform
  __shared__ u64 sC[VOXEL_RAYCAST_COUNTS];
  const int tid = threadIdx.x;
  if (tid < VOXEL_RAYCAST_COUNTS) sC[tid] = 0;
  __syncthreads();
  u64 b[5];
#pragma unroll
  for (int c = 0; c < 5; ++c) b[c] = __ballot(code == c);
  const u64 bk = __ballot(kept);
  unsigned s = code >= 0 ? steps : 0u;  // at most 6,144 per ray: a wavefront's sum fits
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if ((tid & 63) == 0) {
#pragma unroll
    for (int c = 0; c < 5; ++c)
      if (b[c]) atomicAdd(&sC[c], (u64)__popcll(b[c]));
    if (s) atomicAdd(&sC[5], (u64)s);
    if (bk) atomicAdd(&sC[6], (u64)__popcll(bk));
  }
  __syncthreads();
  if (tid < words && sC[tid]) __hip_atomic_fetch_add(&counts[tid], sC[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct VoxelRaysArgs {
  const svo_voxel_ray* rays;
  int n, min_step;
  float voxel_size;
  int o[3], d[3];
  const u64 *bits, *coarse;
  svo_voxel_ray_hit* hits;
  u64* counts;
};

template <bool SKIP>
__global__ __launch_bounds__(VR_T) void voxel_rays_kernel(VoxelRaysArgs a) {
  const int i = (int)blockIdx.x * VR_T + (int)threadIdx.x;
  int code = -1;
  unsigned steps = 0;
  if (i < a.n) {
    const float4 lo = reinterpret_cast<const float4*>(a.rays)[2 * (size_t)i], hi = reinterpret_cast<const float4*>(a.rays)[2 * (size_t)i + 1];
    svo_voxel_ray ray;
    ray.ox = lo.x; ray.oy = lo.y; ray.oz = lo.z; ray.max_range = lo.w;
    ray.dx = hi.x; ray.dy = hi.y; ray.dz = hi.z; ray.tag = 0;
    VoxelRaySetup s;
    svo_voxel_ray_hit h;
    if (voxel_ray_setup_record(ray, a.voxel_size, a.o, &s)) {
      const VoxelRayEnd e = voxel_ray_walk<SKIP>(s, a.d, reinterpret_cast<const uint64_t*>(a.bits), reinterpret_cast<const uint64_t*>(a.coarse), a.min_step);
      h = voxel_ray_result(e, s, a.voxel_size);
      code = e.code; steps = e.steps;
    } else {
      h.cell = VOXEL_RAY_NO_CELL; h.steps = 0; h.dist = 0.0f; h.status = (uint32_t)VOXEL_RAY_REJECTED | 3u << 8;
      code = VOXEL_RAY_REJECTED;
    }
    reinterpret_cast<uint4*>(a.hits)[i] = make_uint4(h.cell, h.steps, __float_as_uint(h.dist), h.status);
  }
  vr_count(a.counts, VOXEL_RAYS_COUNTS, code, steps, false);
}

struct VoxelRaycastArgs {
  int width, height, min_step;
  float voxel_size;
  double focal, cx, cy, baseline, max_range;
  double m[12];
  int o[3], d[3];
  const u64 *bits, *coarse;
  short* disp16;
  unsigned* cell;
  u64* counts;
};

template <bool SKIP>
__global__ __launch_bounds__(VR_T) void voxel_raycast_kernel(VoxelRaycastArgs a) {
  const unsigned tiles_x = ((unsigned)a.width + 7u) >> 3, tiles_y = ((unsigned)a.height + 7u) >> 3;
  const unsigned tile = blockIdx.x * (VR_T / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  const int x = (int)(tile % tiles_x * 8u + (lane & 7u)), y = (int)(tile / tiles_x * 8u + (lane >> 3));
  int code = -1;
  unsigned steps = 0;
  bool kept = false;
  if (tile < tiles_x * tiles_y && x < a.width && y < a.height) {
    double o[3], d[3];
    voxel_pixel_ray(a.m, a.focal, a.cx, a.cy, x, y, o, d);
    VoxelRaySetup s;
    int v = -16;
    unsigned cell = VOXEL_RAY_NO_CELL;
    if (voxel_ray_setup(o, d, a.max_range, a.voxel_size, a.o, &s)) {
      const VoxelRayEnd e = voxel_ray_walk<SKIP>(s, a.d, reinterpret_cast<const uint64_t*>(a.bits), reinterpret_cast<const uint64_t*>(a.coarse), a.min_step);
      v = voxel_ray_disp16(e, s, a.voxel_size, a.focal, a.baseline);
      code = e.code; steps = e.steps;
      kept = v != -16;
      if (kept) cell = e.cell;
    } else {
      code = VOXEL_RAY_REJECTED;
    }
    const size_t px = (size_t)y * (size_t)a.width + (size_t)x;
    a.disp16[px] = (short)v;
    if (a.cell) a.cell[px] = cell;
  }
  vr_count(a.counts, VOXEL_RAYCAST_COUNTS, code, steps, kept);
}
}  // namespace

// ----------------------------------------------------------------------------- host side
extern "C" int svo_voxel_raycast_default_params(svo_voxel_raycast_params* params) { return voxel_raycast_default_params(params); }
extern "C" int svo_voxel_occupancy_coarse_bytes(const int* dims3, size_t* bytes) { return voxel_coarse_bytes(dims3, bytes); }

extern "C" int svo_voxel_occupancy_coarse_dev(svo_voxel_map* m, const uint64_t* bits, const int* dims3, uint64_t* coarse) {
  if (!m) return SVO_ERR_INVALID;
  svo_ctx* ctx = svo_voxel_map_view(m).ctx;
  svo_use_device(ctx);
  SVO_ARGS_CHECK(ctx, voxel_coarse_check(bits, dims3, coarse, &err));
  SvoProfScope prof(ctx, SVO_PROF_VOXEL_COARSE);
  SVO_HIP_CHECK(ctx, hipMemsetAsync(coarse, 0, 8 * voxel_coarse_words(dims3), ctx->stream));
  VoxelCoarseArgs a{};
  a.bits = reinterpret_cast<const u64*>(bits);
  a.coarse = reinterpret_cast<u64*>(coarse);
  a.words = voxel_occupancy_words(dims3);
  a.wpr = dims3[0] >> 6; a.d1 = dims3[1];
  a.cd0 = dims3[0] >> 3; a.cd1 = (dims3[1] + 7) >> 3;
  hipLaunchKernelGGL(voxel_coarse_kernel, dim3((unsigned)voxel_coarse_groups(dims3)), dim3(VR_CT), 0, ctx->stream, a);
  SVO_HIP_CHECK(ctx, hipGetLastError());
  return SVO_OK;
}

// The counts' memset and the launch of checked arguments.
static int voxel_rays_launch(const SvoVoxelView& t, const uint64_t* bits, const uint64_t* coarse, const int* origin, const int* dims, const svo_voxel_ray* rays,
                             int n, int min_step, svo_voxel_ray_hit* hits, uint64_t* counts) {
  svo_ctx* ctx = t.ctx;
  SvoProfScope prof(ctx, SVO_PROF_VOXEL_RAYS);
  if (counts) SVO_HIP_CHECK(ctx, hipMemsetAsync(counts, 0, VOXEL_RAYS_COUNTS * sizeof(uint64_t), ctx->stream));
  if (n == 0) return SVO_OK;
  VoxelRaysArgs a{};
  a.rays = rays; a.n = n; a.min_step = min_step;
  a.voxel_size = t.voxel_size;
  for (int r = 0; r < 3; ++r) { a.o[r] = origin[r]; a.d[r] = dims[r]; }
  a.bits = reinterpret_cast<const u64*>(bits);
  a.coarse = reinterpret_cast<const u64*>(coarse);
  a.hits = hits;
  a.counts = reinterpret_cast<u64*>(counts);
  const dim3 grid((unsigned)voxel_rays_groups(n)), block(VR_T);
  if (coarse) hipLaunchKernelGGL(voxel_rays_kernel<true>, grid, block, 0, ctx->stream, a);
  else hipLaunchKernelGGL(voxel_rays_kernel<false>, grid, block, 0, ctx->stream, a);
  SVO_HIP_CHECK(ctx, hipGetLastError());
  return SVO_OK;
}

extern "C" int svo_voxel_occupancy_rays_dev(svo_voxel_map* m, const uint64_t* bits, const uint64_t* coarse, const int* origin3, const int* dims3,
                                            const svo_voxel_ray* rays, int n, int min_step, svo_voxel_ray_hit* hits, uint64_t* counts) {
  if (!m) return SVO_ERR_INVALID;
  const SvoVoxelView t = svo_voxel_map_view(m);
  svo_use_device(t.ctx);
  SVO_ARGS_CHECK(t.ctx, voxel_rays_check(bits, coarse, origin3, dims3, rays, n, min_step, hits, counts, true, &err));
  return voxel_rays_launch(t, bits, coarse, origin3, dims3, rays, n, min_step, hits, counts);
}

extern "C" int svo_voxel_occupancy_rays(svo_voxel_map* m, const uint64_t* bits, const uint64_t* coarse, const int* origin3, const int* dims3,
                                        const svo_voxel_ray* host_rays, int n, int min_step, svo_voxel_ray_hit* host_hits, uint64_t* host_counts) {
  if (!m) return SVO_ERR_INVALID;
  const SvoVoxelView t = svo_voxel_map_view(m);
  svo_ctx* ctx = t.ctx;
  svo_use_device(ctx);
  SVO_ARGS_CHECK(ctx, voxel_rays_check(bits, coarse, origin3, dims3, host_rays, n, min_step, host_hits, host_counts, false, &err));
  const size_t rbytes = sizeof(svo_voxel_ray) * (size_t)n, hbytes = sizeof(svo_voxel_ray_hit) * (size_t)n;
  SvoParts parts;
  const size_t o_counts = parts.add(VOXEL_RAYS_COUNTS * sizeof(uint64_t)), o_rays = parts.add(rbytes), o_hits = parts.add(hbytes);
  SvoTemp d;
  SVO_HIP_CHECK(ctx, hipMalloc(&d.p, parts.total()));
  uint64_t c[VOXEL_RAYS_COUNTS] = {};
  const int rc = svo_host_call(
      ctx, "voxel_occupancy_rays", n ? hipMemcpyAsync(d.at(o_rays), host_rays, rbytes, hipMemcpyHostToDevice, ctx->stream) : hipSuccess,
      [&] {
        return voxel_rays_launch(t, bits, coarse, origin3, dims3, d.at<svo_voxel_ray>(o_rays), n, min_step, d.at<svo_voxel_ray_hit>(o_hits),
                                 d.at<uint64_t>(o_counts));
      },
      [&] {
        hipError_t e = n ? hipMemcpyAsync(host_hits, d.at(o_hits), hbytes, hipMemcpyDeviceToHost, ctx->stream) : hipSuccess;
        if (e == hipSuccess && host_counts) e = hipMemcpyAsync(c, d.at(o_counts), sizeof(c), hipMemcpyDeviceToHost, ctx->stream);
        return e;
      });
  if (rc) return rc;
  if (host_counts) memcpy(host_counts, c, sizeof(c));
  return SVO_OK;
}

extern "C" int svo_voxel_occupancy_raycast_dev(svo_voxel_map* m, const uint64_t* bits, const uint64_t* coarse, const int* origin3, const int* dims3,
                                               int width, int height, const svo_camera_info* cam, const double* c2w12,
                                               const svo_voxel_raycast_params* prm, int16_t* disp16, uint32_t* cell, uint64_t* counts) {
  if (!m) return SVO_ERR_INVALID;
  const SvoVoxelView t = svo_voxel_map_view(m);
  svo_ctx* ctx = t.ctx;
  svo_use_device(ctx);
  SVO_ARGS_CHECK(ctx, voxel_raycast_check(bits, coarse, origin3, dims3, width, height, cam, c2w12, prm, ctx->lim.max_width, ctx->lim.max_height, disp16,
                                            cell, counts, &err));
  SvoProfScope prof(ctx, SVO_PROF_VOXEL_RAYS);
  if (counts) SVO_HIP_CHECK(ctx, hipMemsetAsync(counts, 0, VOXEL_RAYCAST_COUNTS * sizeof(uint64_t), ctx->stream));
  VoxelRaycastArgs a{};
  a.width = width; a.height = height; a.min_step = prm->min_step;
  a.voxel_size = t.voxel_size;
  a.focal = cam->focal; a.cx = cam->cx; a.cy = cam->cy; a.baseline = cam->baseline;
  a.max_range = (double)prm->max_range;
  memcpy(a.m, c2w12, sizeof(a.m));
  for (int r = 0; r < 3; ++r) { a.o[r] = origin3[r]; a.d[r] = dims3[r]; }
  a.bits = reinterpret_cast<const u64*>(bits);
  a.coarse = reinterpret_cast<const u64*>(coarse);
  a.disp16 = disp16; a.cell = cell;
  a.counts = reinterpret_cast<u64*>(counts);
  const dim3 grid((unsigned)voxel_raycast_groups(width, height)), block(VR_T);
  if (coarse) hipLaunchKernelGGL(voxel_raycast_kernel<true>, grid, block, 0, ctx->stream, a);
  else hipLaunchKernelGGL(voxel_raycast_kernel<false>, grid, block, 0, ctx->stream, a);
  SVO_HIP_CHECK(ctx, hipGetLastError());
  return SVO_OK;
}

extern "C" int svo_voxel_occupancy_raycast_pose7_dev(svo_voxel_map* m, const uint64_t* bits, const uint64_t* coarse, const int* origin3, const int* dims3,
                                                     int width, int height, const svo_camera_info* cam, const double* pose7,
                                                     const svo_voxel_raycast_params* prm, int16_t* disp16, uint32_t* cell, uint64_t* counts) {
  if (!m) return SVO_ERR_INVALID;
  svo_ctx* ctx = svo_voxel_map_view(m).ctx;
  SVO_REQUIRE(ctx, cam, "voxel_occupancy_raycast: null cam");
  SVO_REQUIRE(ctx, pose7, "voxel_occupancy_raycast_pose7: null pose7");
  double m12[12];
  voxel_pose7_to_cam_to_world(pose7, m12);
  return svo_voxel_occupancy_raycast_dev(m, bits, coarse, origin3, dims3, width, height, cam, m12, prm, disp16, cell, counts);
}

extern "C" int svo_voxel_map_raycast(svo_voxel_map* m, int min_count, const int* dims3, int width, int height, const svo_camera_info* cam,
                                     const double* c2w12, const svo_voxel_raycast_params* prm, int16_t* disp16, uint32_t* cell, uint64_t* counts,
                                     int* origin3_out) {
  if (!m) return SVO_ERR_INVALID;
  const SvoVoxelView t = svo_voxel_map_view(m);
  svo_ctx* ctx = t.ctx;
  svo_use_device(ctx);
  SVO_ARGS_CHECK(ctx, voxel_map_raycast_check(min_count, dims3, width, height, cam, c2w12, prm, ctx->lim.max_width, ctx->lim.max_height, disp16, &err));
  const double T[3] = {c2w12[3], c2w12[7], c2w12[11]};
  int origin[3];
  SVO_ARGS_CHECK(ctx, voxel_locate_origin(T, t.voxel_size, dims3, origin, &err));
  if (origin3_out) memcpy(origin3_out, origin, sizeof(origin));
  const size_t px = (size_t)width * (size_t)height;
  SvoParts parts;  // the occupancy's two u32 counts are asked for and dropped
  const size_t o_bits = parts.add(8 * voxel_occupancy_words(dims3)), o_coarse = parts.add(8 * voxel_coarse_words(dims3)),
               o_counts = parts.add(VOXEL_RAYCAST_COUNTS * sizeof(uint64_t)), o_occ = parts.add(2 * sizeof(uint32_t)), o_disp = parts.add(2 * px),
               o_cell = parts.add(4 * px);
  SvoTemp d;
  SVO_HIP_CHECK(ctx, hipMalloc(&d.p, parts.total()));
  uint64_t* const d_bits = d.at<uint64_t>(o_bits);
  uint64_t* const d_coarse = VOXEL_RAYCAST_HOST_SKIPS ? d.at<uint64_t>(o_coarse) : nullptr;
  uint64_t c[VOXEL_RAYCAST_COUNTS] = {};
  const int rc = svo_host_call(
      ctx, "voxel_map_raycast", hipSuccess,
      [&] {
        int rc = svo_voxel_map_occupancy_dev(m, min_count, origin, dims3, d_bits, d.at<uint32_t>(o_occ));
        if (!rc && d_coarse) rc = svo_voxel_occupancy_coarse_dev(m, d_bits, dims3, d_coarse);
        if (!rc) rc = svo_voxel_occupancy_raycast_dev(m, d_bits, d_coarse, origin, dims3, width, height, cam, c2w12, prm, d.at<int16_t>(o_disp),
                                                      cell ? d.at<uint32_t>(o_cell) : nullptr, d.at<uint64_t>(o_counts));
        return rc;
      },
      [&] {
        hipError_t e = hipMemcpyAsync(disp16, d.at(o_disp), 2 * px, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess && cell) e = hipMemcpyAsync(cell, d.at(o_cell), 4 * px, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess && counts) e = hipMemcpyAsync(c, d.at(o_counts), sizeof(c), hipMemcpyDeviceToHost, ctx->stream);
        return e;
      });
  if (rc) return rc;
  if (counts) memcpy(counts, c, sizeof(c));
  return SVO_OK;
}
