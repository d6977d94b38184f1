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
#define VOXEL_RAYS_CHECK(ctx, call) do { const char* err = nullptr; if (call) { (ctx)->err = err; return SVO_ERR_INVALID; } } while (0)

extern "C" int svo_voxel_raycast_default_params(svo_voxel_raycast_params* params) { return voxel_raycast_default_params(params); }
extern "C" int svo_voxel_occupancy_coarse_bytes(const int* dims3, size_t* bytes) { return voxel_coarse_bytes(dims3, bytes); }

extern "C" int svo_voxel_occupancy_coarse_dev(svo_voxel_map* m, const uint64_t* bits, const int* dims3, uint64_t* coarse) {
  if (!m) return SVO_ERR_INVALID;
  svo_ctx* ctx = svo_voxel_map_view(m).ctx;
  svo_use_device(ctx);
  VOXEL_RAYS_CHECK(ctx, voxel_coarse_check(bits, dims3, coarse, &err));
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
  VOXEL_RAYS_CHECK(t.ctx, voxel_rays_check(bits, coarse, origin3, dims3, rays, n, min_step, hits, counts, true, &err));
  return voxel_rays_launch(t, bits, coarse, origin3, dims3, rays, n, min_step, hits, counts);
}

extern "C" int svo_voxel_occupancy_rays(svo_voxel_map* m, const uint64_t* bits, const uint64_t* coarse, const int* origin3, const int* dims3,
                                        const svo_voxel_ray* host_rays, int n, int min_step, svo_voxel_ray_hit* host_hits, uint64_t* host_counts) {
  if (!m) return SVO_ERR_INVALID;
  const SvoVoxelView t = svo_voxel_map_view(m);
  svo_ctx* ctx = t.ctx;
  svo_use_device(ctx);
  VOXEL_RAYS_CHECK(ctx, voxel_rays_check(bits, coarse, origin3, dims3, host_rays, n, min_step, host_hits, host_counts, false, &err));
  const size_t cbytes = 256, rbytes = sizeof(svo_voxel_ray) * (size_t)n, hbytes = sizeof(svo_voxel_ray_hit) * (size_t)n;  // counts | rays | hits
  char* d = nullptr;
  SVO_HIP_CHECK(ctx, hipMalloc(reinterpret_cast<void**>(&d), cbytes + rbytes + hbytes));
  svo_voxel_ray* d_rays = reinterpret_cast<svo_voxel_ray*>(d + cbytes);
  svo_voxel_ray_hit* d_hits = reinterpret_cast<svo_voxel_ray_hit*>(d + cbytes + rbytes);
  hipError_t e = n ? hipMemcpyAsync(d_rays, host_rays, rbytes, hipMemcpyHostToDevice, ctx->stream) : hipSuccess;
  int rc = SVO_OK;
  if (e == hipSuccess) rc = voxel_rays_launch(t, bits, coarse, origin3, dims3, d_rays, n, min_step, d_hits, reinterpret_cast<uint64_t*>(d));
  if (!rc && e == hipSuccess && n) e = hipMemcpyAsync(host_hits, d_hits, hbytes, hipMemcpyDeviceToHost, ctx->stream);
  if (!rc && e == hipSuccess && host_counts) e = hipMemcpyAsync(host_counts, d, VOXEL_RAYS_COUNTS * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream);
  const hipError_t e2 = hipStreamSynchronize(ctx->stream);
  (void)hipFree(d);
  if (rc) return rc;
  if (e == hipSuccess) e = e2;
  if (e != hipSuccess) { ctx->err = std::string("voxel_occupancy_rays: ") + hipGetErrorString(e); return SVO_ERR_HIP; }
  return SVO_OK;
}

extern "C" int svo_voxel_occupancy_raycast_dev(svo_voxel_map* m, const uint64_t* bits, const uint64_t* coarse, const int* origin3, const int* dims3,
                                               int width, int height, const svo_camera_info* cam, const double* c2w12,
                                               const svo_voxel_raycast_params* prm, int16_t* disp16, uint32_t* cell, uint64_t* counts) {
  if (!m) return SVO_ERR_INVALID;
  const SvoVoxelView t = svo_voxel_map_view(m);
  svo_ctx* ctx = t.ctx;
  svo_use_device(ctx);
  VOXEL_RAYS_CHECK(ctx, voxel_raycast_check(bits, coarse, origin3, dims3, width, height, cam, c2w12, prm, ctx->lim.max_width, ctx->lim.max_height, disp16,
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
  VOXEL_RAYS_CHECK(ctx, voxel_map_raycast_check(min_count, dims3, width, height, cam, c2w12, prm, ctx->lim.max_width, ctx->lim.max_height, disp16, &err));
  const double T[3] = {c2w12[3], c2w12[7], c2w12[11]};
  int origin[3];
  VOXEL_RAYS_CHECK(ctx, voxel_locate_origin(T, t.voxel_size, dims3, origin, &err));
  if (origin3_out) memcpy(origin3_out, origin, sizeof(origin));
  const size_t px = (size_t)width * (size_t)height, r256 = 255;
  const size_t bbytes = 8 * voxel_occupancy_words(dims3), cbytes = (8 * voxel_coarse_words(dims3) + r256) & ~r256;
  const size_t dbytes = (2 * px + r256) & ~r256, lbytes = 4 * px;  // volume | coarse | counts | disp16 | cell
  char* d = nullptr;
  SVO_HIP_CHECK(ctx, hipMalloc(reinterpret_cast<void**>(&d), bbytes + cbytes + 256 + dbytes + lbytes));
  uint64_t *d_bits = reinterpret_cast<uint64_t*>(d), *d_coarse = reinterpret_cast<uint64_t*>(d + bbytes);
  uint64_t* d_counts = reinterpret_cast<uint64_t*>(d + bbytes + cbytes);  // seven words, and the occupancy's two u32 behind them
  int16_t* d_disp = reinterpret_cast<int16_t*>(d + bbytes + cbytes + 256);
  uint32_t* d_cell = reinterpret_cast<uint32_t*>(d + bbytes + cbytes + 256 + dbytes);
  int rc = svo_voxel_map_occupancy_dev(m, min_count, origin, dims3, d_bits, reinterpret_cast<uint32_t*>(d_counts + 8));
  if (!rc && VOXEL_RAYCAST_HOST_SKIPS) rc = svo_voxel_occupancy_coarse_dev(m, d_bits, dims3, d_coarse);
  if (!rc) rc = svo_voxel_occupancy_raycast_dev(m, d_bits, VOXEL_RAYCAST_HOST_SKIPS ? d_coarse : nullptr, origin, dims3, width, height, cam, c2w12, prm, d_disp,
                                                cell ? d_cell : nullptr, d_counts);
  hipError_t e = hipSuccess;
  if (!rc) e = hipMemcpyAsync(disp16, d_disp, 2 * px, hipMemcpyDeviceToHost, ctx->stream);
  if (!rc && e == hipSuccess && cell) e = hipMemcpyAsync(cell, d_cell, 4 * px, hipMemcpyDeviceToHost, ctx->stream);
  if (!rc && e == hipSuccess && counts) e = hipMemcpyAsync(counts, d_counts, VOXEL_RAYCAST_COUNTS * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream);
  const hipError_t e2 = hipStreamSynchronize(ctx->stream);
  (void)hipFree(d);
  if (rc) return rc;
  if (e == hipSuccess) e = e2;
  if (e != hipSuccess) { ctx->err = std::string("voxel_map_raycast: ") + hipGetErrorString(e); return SVO_ERR_HIP; }
  return SVO_OK;
}
