// Voxel map distance field (include/svo.h, "Voxel map distance field"): per cell of the occupancy entry's dense bit
// volume the exact squared distance to the nearest set bit, that bit's number, the distance in map units and the volume inflated
// by a radius, in three launches on the map's stream; and a per-sphere query of the field.
//
//   voxel_distance_row_kernel    : axis 0, bit-parallel.  One thread per cell, lanes along j0, so a wavefront's 64 cells are one u64
//                                  word and every load is wavefront-uniform (the word index goes through readfirstlane; the loads
//                                  are scalar).  host/voxel_distance.h's voxel_distance_row: mask + clz to the left, shift + ctz to
//                                  the right, then the row's neighbouring words outward.  Writes the |offset| (u8) or, in the form
//                                  with `nearest`, the signed offset (i16).
//   voxel_distance_column_kernel : axes 1 and 2 (LAST), §7k's column pass.  One thread per cell, lanes along j0, so every step's
//                                  loads are one or two lines per wavefront.  The search is the header's voxel_distance_column,
//                                  four steps' loads issued before the first test.  The axis-1 launch writes the partial square
//                                  (u16) or both offsets packed (u32); the axis-2 launch applies the cap and writes dist2, the
//                                  optional outputs and - one ballot per wavefront, lane 0 storing it - the inflated word.
//   voxel_distance_query_kernel  : one sphere per lane, the header's voxel_distance_query_one, one 16-byte store.
// Each kernel but the last exists in two forms, NEAR = false (out->nearest == NULL: nothing carries an index) and true.
//
// §7c's conditions: relaxed device-scope atomics only (the counts: ballots, LDS, one add per workgroup and non-zero counter), no
// fence, no waiting on another workgroup, every output element written by exactly one thread, the passes ping-pong between two
// parts of the workspace, size_t offsets (d0 * d1 * d2 reaches 2^30).  Bounds: the cell count is a multiple of 64, so a wavefront
// is whole or absent; a row's words are x - k >= 0 and x + k < wpr; a line's positions are clamped into [0, len).
#include "kernels.h"
#include "voxel_distance.h"

namespace {
typedef unsigned long long u64;
constexpr int VD_T = VOXEL_DISTANCE_THREADS;

struct VoxelDistanceRowArgs {
  const u64* bits;
  void* out;  // u8 or i16 per cell
  size_t n;
  int wpr, max_dist;
};

template <bool NEAR>
__global__ __launch_bounds__(VD_T) void voxel_distance_row_kernel(VoxelDistanceRowArgs a) {
  const size_t i = (size_t)blockIdx.x * VD_T + (size_t)threadIdx.x;
  if (i >= a.n) return;  // whole wavefronts: n is a multiple of 64
  const unsigned word = __builtin_amdgcn_readfirstlane((unsigned)(i >> 6));  // below 2^24
  const unsigned row = word / (unsigned)a.wpr, x = word - row * (unsigned)a.wpr;
  const int off = voxel_distance_row(reinterpret_cast<const uint64_t*>(a.bits) + (size_t)row * (size_t)a.wpr, a.wpr, (int)x, (int)(threadIdx.x & 63u), a.max_dist);
  if (NEAR) static_cast<int16_t*>(a.out)[i] = (int16_t)off;
  else static_cast<uint8_t*>(a.out)[i] = off == VOXEL_DISTANCE_NO_OFFSET ? (uint8_t)255 : (uint8_t)(off < 0 ? -off : off);
}

struct VoxelDistanceColumnArgs {
  const void* in;
  void* mid;  // the axis-1 launch's output
  size_t n;
  int d0, d1, d2, max_dist;
  uint32_t r2;
  float voxel_size;
  svo_voxel_distance_out o;  // the axis-2 launch's
  u64* counts;
};

template <bool NEAR, bool LAST>
__global__ __launch_bounds__(VD_T) void voxel_distance_column_kernel(VoxelDistanceColumnArgs a) {
  typedef typename VoxelDistanceIn<NEAR, LAST>::T In;
  __shared__ unsigned sC[VOXEL_DISTANCE_COUNTS][VD_T / 64];
  const int tid = threadIdx.x;
  const size_t i = (size_t)blockIdx.x * VD_T + (size_t)tid;
  u64 b_src = 0, b_none = 0, b_infl = 0, b_all = 0;
  if (i < a.n) {
    const unsigned rest = (unsigned)i / (unsigned)a.d0;  // i < 2^30: 32-bit divisions
    const int j2 = (int)(rest / (unsigned)a.d1), j1 = (int)(rest - (unsigned)j2 * (unsigned)a.d1);
    const size_t stride = LAST ? (size_t)a.d0 * (size_t)a.d1 : (size_t)a.d0;
    const int p = LAST ? j2 : j1, len = LAST ? a.d2 : a.d1;
    const size_t line0 = i - (size_t)p * stride;
    const VoxelDistanceBest r = voxel_distance_column<NEAR, LAST>(static_cast<const In*>(a.in) + line0, stride, p, len, a.max_dist, (uint32_t)line0, a.d0);
    if (!LAST) {
      if (NEAR) static_cast<uint32_t*>(a.mid)[i] = r.arg;
      else static_cast<uint16_t*>(a.mid)[i] = r.d2 == VOXEL_DISTANCE_NONE ? VOXEL_DISTANCE_NONE16 : (uint16_t)r.d2;
    } else {
      const bool none = r.d2 == VOXEL_DISTANCE_NONE, infl = r.d2 <= a.r2;  // NONE is above every R2
      a.o.dist2[i] = none ? VOXEL_DISTANCE_NONE16 : (uint16_t)r.d2;
      if (NEAR) a.o.nearest[i] = r.at;
      if (a.o.clearance) a.o.clearance[i] = voxel_distance_clearance(r.d2, a.voxel_size);
      b_infl = __ballot(infl);
      if (a.o.inflated && (tid & 63) == 0) a.o.inflated[i >> 6] = b_infl;
      b_src = __ballot(r.d2 == 0u);
      b_none = __ballot(none);
      b_all = ~0ull;
    }
  }
  if (!LAST || !a.counts) return;  // uniform over the launch
  if ((tid & 63) == 0) {
    sC[0][tid >> 6] = (unsigned)__popcll(b_src);
    sC[1][tid >> 6] = (unsigned)(__popcll(b_all) - __popcll(b_src) - __popcll(b_none));
    sC[2][tid >> 6] = (unsigned)__popcll(b_none);
    sC[3][tid >> 6] = (unsigned)__popcll(b_infl);
  }
  __syncthreads();
  if (tid < VOXEL_DISTANCE_COUNTS) {
    unsigned t = 0;
    for (int w = 0; w < VD_T / 64; ++w) t += sC[tid][w];
    if (t) __hip_atomic_fetch_add(&a.counts[tid], (u64)t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

struct VoxelDistanceQueryArgs {
  const uint16_t* dist2;
  const svo_voxel_sphere* spheres;
  svo_voxel_sphere_hit* hits;
  u64* counts;
  int n;
  float voxel_size;
  int o[3], d[3];
};

__global__ __launch_bounds__(VD_T) void voxel_distance_query_kernel(VoxelDistanceQueryArgs a) {
  __shared__ unsigned sC[VOXEL_DISTANCE_QUERY_COUNTS][VD_T / 64];
  const int tid = threadIdx.x;
  const int i = (int)blockIdx.x * VD_T + tid;
  int code = -1;
  bool beyond = false;
  if (i < a.n) {
    const float4 s4 = reinterpret_cast<const float4*>(a.spheres)[i];
    const float s[4] = {s4.x, s4.y, s4.z, s4.w};
    const svo_voxel_sphere_hit h = voxel_distance_query_one(s, a.voxel_size, a.o, a.d, a.dist2, &beyond);
    reinterpret_cast<uint4*>(a.hits)[i] = make_uint4(h.cell, h.dist2, __float_as_uint(h.clearance), h.code);
    code = (int)h.code;
  }
  if (!a.counts) return;  // uniform over the launch
  u64 b[VOXEL_DISTANCE_QUERY_COUNTS];
  b[0] = __ballot(code >= 0);
#pragma unroll
  for (int c = 0; c < 4; ++c) b[1 + c] = __ballot(code == c);
  b[5] = __ballot(beyond);
  if ((tid & 63) == 0) {
#pragma unroll
    for (int c = 0; c < VOXEL_DISTANCE_QUERY_COUNTS; ++c) sC[c][tid >> 6] = (unsigned)__popcll(b[c]);
  }
  __syncthreads();
  if (tid < VOXEL_DISTANCE_QUERY_COUNTS) {
    unsigned t = 0;
    for (int w = 0; w < VD_T / 64; ++w) t += sC[tid][w];
    if (t) __hip_atomic_fetch_add(&a.counts[tid], (u64)t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

template <bool NEAR>
void voxel_distance_launches(hipStream_t st, dim3 grid, const VoxelDistanceRowArgs& ra, const VoxelDistanceColumnArgs& c1, const VoxelDistanceColumnArgs& c2) {
  hipLaunchKernelGGL(voxel_distance_row_kernel<NEAR>, grid, dim3(VD_T), 0, st, ra);
  hipLaunchKernelGGL((voxel_distance_column_kernel<NEAR, false>), grid, dim3(VD_T), 0, st, c1);
  hipLaunchKernelGGL((voxel_distance_column_kernel<NEAR, true>), grid, dim3(VD_T), 0, st, c2);
}
}  // namespace

// ----------------------------------------------------------------------------- host side
extern "C" int svo_voxel_distance_default_params(float voxel_size, svo_voxel_distance_params* out) { return voxel_distance_default_params(voxel_size, out); }
extern "C" int svo_voxel_distance_workspace_bytes(const int* dims3, int want_nearest, size_t* bytes) { return voxel_distance_workspace_bytes(dims3, want_nearest, bytes); }
extern "C" int svo_voxel_distance_bytes(const int* dims3, size_t* bytes) { return voxel_distance_bytes(dims3, bytes); }

extern "C" int svo_voxel_occupancy_distance_dev(svo_voxel_map* m, const uint64_t* bits, const int* dims3, const svo_voxel_distance_params* prm,
                                                void* workspace, const svo_voxel_distance_out* out, uint64_t* counts) {
  if (!m) return SVO_ERR_INVALID;
  const SvoVoxelView t = svo_voxel_map_view(m);
  svo_ctx* ctx = t.ctx;
  svo_use_device(ctx);
  SVO_ARGS_CHECK(ctx, voxel_distance_check(bits, dims3, prm, workspace, out, counts, &err));
  const bool near = out->nearest != nullptr;
  const VoxelDistanceLayout lay = voxel_distance_layout(dims3, near);
  char* const ws = static_cast<char*>(workspace);
  VoxelDistanceRowArgs ra{};
  ra.bits = reinterpret_cast<const u64*>(bits);
  ra.out = ws;
  ra.n = voxel_distance_cells(dims3);
  ra.wpr = dims3[0] >> 6; ra.max_dist = prm->max_dist;
  VoxelDistanceColumnArgs c1{};
  c1.in = ws; c1.mid = ws + lay.second;
  c1.n = ra.n;
  c1.d0 = dims3[0]; c1.d1 = dims3[1]; c1.d2 = dims3[2]; c1.max_dist = prm->max_dist;
  VoxelDistanceColumnArgs c2 = c1;
  c2.in = c1.mid; c2.mid = nullptr;
  c2.r2 = voxel_distance_r2(prm->inflate_radius, t.voxel_size, prm->max_dist);
  c2.voxel_size = t.voxel_size;
  c2.o = *out;
  c2.counts = reinterpret_cast<u64*>(counts);
  const dim3 grid((unsigned)voxel_distance_groups(dims3));
  SvoProfScope prof(ctx, SVO_PROF_VOXEL_DISTANCE);
  if (counts) SVO_HIP_CHECK(ctx, hipMemsetAsync(counts, 0, VOXEL_DISTANCE_COUNTS * sizeof(uint64_t), ctx->stream));
  if (near) voxel_distance_launches<true>(ctx->stream, grid, ra, c1, c2);
  else voxel_distance_launches<false>(ctx->stream, grid, ra, c1, c2);
  SVO_HIP_CHECK(ctx, hipGetLastError());
  return SVO_OK;
}

// The counts' memset and the launch of checked arguments.
static int voxel_distance_query_launch(const SvoVoxelView& t, const uint16_t* dist2, const int* origin, const int* dims, const svo_voxel_sphere* spheres, int n,
                                       svo_voxel_sphere_hit* hits, uint64_t* counts) {
  svo_ctx* ctx = t.ctx;
  SvoProfScope prof(ctx, SVO_PROF_VOXEL_DISTANCE_QUERY);
  if (counts) SVO_HIP_CHECK(ctx, hipMemsetAsync(counts, 0, VOXEL_DISTANCE_QUERY_COUNTS * sizeof(uint64_t), ctx->stream));
  if (n == 0) return SVO_OK;
  VoxelDistanceQueryArgs a{};
  a.dist2 = dist2; a.spheres = spheres; a.hits = hits;
  a.counts = reinterpret_cast<u64*>(counts);
  a.n = n; a.voxel_size = t.voxel_size;
  for (int r = 0; r < 3; ++r) { a.o[r] = origin[r]; a.d[r] = dims[r]; }
  hipLaunchKernelGGL(voxel_distance_query_kernel, dim3((unsigned)voxel_distance_query_groups(n)), dim3(VD_T), 0, ctx->stream, a);
  SVO_HIP_CHECK(ctx, hipGetLastError());
  return SVO_OK;
}

extern "C" int svo_voxel_distance_query_dev(svo_voxel_map* m, const uint16_t* dist2, const int* origin3, const int* dims3, const svo_voxel_sphere* spheres,
                                            int n, svo_voxel_sphere_hit* hits, uint64_t* counts) {
  if (!m) return SVO_ERR_INVALID;
  const SvoVoxelView t = svo_voxel_map_view(m);
  svo_use_device(t.ctx);
  SVO_ARGS_CHECK(t.ctx, voxel_distance_query_check(dist2, origin3, dims3, spheres, n, hits, counts, true, &err));
  return voxel_distance_query_launch(t, dist2, origin3, dims3, spheres, n, hits, counts);
}

extern "C" int svo_voxel_distance_query(svo_voxel_map* m, const uint16_t* dist2, const int* origin3, const int* dims3, const svo_voxel_sphere* host_spheres,
                                        int n, svo_voxel_sphere_hit* host_hits, uint64_t* host_counts) {
  if (!m) return SVO_ERR_INVALID;
  const SvoVoxelView t = svo_voxel_map_view(m);
  svo_ctx* ctx = t.ctx;
  svo_use_device(ctx);
  SVO_ARGS_CHECK(ctx, voxel_distance_query_check(dist2, origin3, dims3, host_spheres, n, host_hits, host_counts, false, &err));
  const size_t sbytes = sizeof(svo_voxel_sphere) * (size_t)n, hbytes = sizeof(svo_voxel_sphere_hit) * (size_t)n;
  SvoParts parts;
  const size_t o_counts = parts.add(VOXEL_DISTANCE_QUERY_COUNTS * sizeof(uint64_t)), o_s = parts.add(sbytes), o_h = parts.add(hbytes);
  SvoTemp d;
  SVO_HIP_CHECK(ctx, hipMalloc(&d.p, parts.total()));
  uint64_t c[VOXEL_DISTANCE_QUERY_COUNTS] = {};
  const int rc = svo_host_call(
      ctx, "voxel_distance_query", n ? hipMemcpyAsync(d.at(o_s), host_spheres, sbytes, hipMemcpyHostToDevice, ctx->stream) : hipSuccess,
      [&] {
        return voxel_distance_query_launch(t, dist2, origin3, dims3, d.at<svo_voxel_sphere>(o_s), n, d.at<svo_voxel_sphere_hit>(o_h), d.at<uint64_t>(o_counts));
      },
      [&] {
        hipError_t e = n ? hipMemcpyAsync(host_hits, d.at(o_h), hbytes, hipMemcpyDeviceToHost, ctx->stream) : hipSuccess;
        if (e == hipSuccess && host_counts) e = hipMemcpyAsync(c, d.at(o_counts), sizeof(c), hipMemcpyDeviceToHost, ctx->stream);
        return e;
      });
  if (rc) return rc;
  if (host_counts) memcpy(host_counts, c, sizeof(c));
  return SVO_OK;
}

extern "C" int svo_voxel_map_distance(svo_voxel_map* m, int min_count, const int* origin3, const int* dims3, const svo_voxel_distance_params* prm,
                                      const svo_voxel_distance_out* host_out, uint64_t* host_counts) {
  if (!m) return SVO_ERR_INVALID;
  const SvoVoxelView t = svo_voxel_map_view(m);
  svo_ctx* ctx = t.ctx;
  svo_use_device(ctx);
  SVO_ARGS_CHECK(ctx, voxel_map_distance_check(min_count, origin3, dims3, prm, host_out, &err));
  const size_t n = voxel_distance_cells(dims3), bbytes = n / 8;
  const bool near = host_out->nearest != nullptr;
  SvoParts parts;  // the occupancy's two u32 counts are asked for and dropped
  const size_t o_counts = parts.add(VOXEL_DISTANCE_COUNTS * sizeof(uint64_t)), o_occ = parts.add(2 * sizeof(uint32_t)), o_bits = parts.add(bbytes),
               o_infl = parts.add(host_out->inflated ? bbytes : 0), o_ws = parts.add(voxel_distance_layout(dims3, near).total), o_d2 = parts.add(2 * n),
               o_near = parts.add(near ? 4 * n : 0), o_clr = parts.add(host_out->clearance ? 4 * n : 0);
  SvoTemp d;
  SVO_HIP_CHECK(ctx, hipMalloc(&d.p, parts.total()));
  svo_voxel_distance_out o{};
  o.dist2 = d.at<uint16_t>(o_d2);
  o.nearest = near ? d.at<uint32_t>(o_near) : nullptr;  // what the caller did not ask for is not written
  o.clearance = host_out->clearance ? d.at<float>(o_clr) : nullptr;
  o.inflated = host_out->inflated ? d.at<uint64_t>(o_infl) : nullptr;
  uint64_t c[VOXEL_DISTANCE_COUNTS] = {};
  const int rc = svo_host_call(
      ctx, "voxel_map_distance", hipSuccess,
      [&] {
        const int rc = svo_voxel_map_occupancy_dev(m, min_count, origin3, dims3, d.at<uint64_t>(o_bits), d.at<uint32_t>(o_occ));
        return rc ? rc : svo_voxel_occupancy_distance_dev(m, d.at<uint64_t>(o_bits), dims3, prm, d.at(o_ws), &o, d.at<uint64_t>(o_counts));
      },
      [&] {
        hipError_t e = hipMemcpyAsync(host_out->dist2, o.dist2, 2 * n, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess && near) e = hipMemcpyAsync(host_out->nearest, o.nearest, 4 * n, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess && o.clearance) e = hipMemcpyAsync(host_out->clearance, o.clearance, 4 * n, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess && o.inflated) e = hipMemcpyAsync(host_out->inflated, o.inflated, bbytes, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess && host_counts) e = hipMemcpyAsync(c, d.at(o_counts), sizeof(c), hipMemcpyDeviceToHost, ctx->stream);
        return e;
      });
  if (rc) return rc;
  if (host_counts) memcpy(host_counts, c, sizeof(c));
  return SVO_OK;
}
