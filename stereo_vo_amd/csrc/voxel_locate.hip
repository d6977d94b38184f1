// Voxel map locate (include/svo.h, "Voxel map locate"): a dense bit volume of the map around a prior, and the number of
// records of a cloud that land in live voxels for every candidate rotation and every whole-voxel shift of a box.
//
//   voxel_occupancy_kernel     : one thread per slot, 1,024-thread workgroups.  A qualifying slot inside the volume sets its bit by a
//                                relaxed atomicOr; the two counts go through a ballot and LDS, one relaxed atomicAdd per workgroup
//                                and non-zero count.
//   voxel_locate_scores_kernel : the bit-sliced form.  A workgroup takes one candidate (blockIdx.y) and a chunk of VOXEL_LOCATE_CHUNK
//                                records (blockIdx.x).  Phase 1 transforms the chunk's records and stages their j into LDS (a record
//                                that is rejected, or that no shift of the box can bring into the volume, is staged as a sentinel no
//                                row accepts).  Phase 2: a work item is a row (s_1, s_2) of the box and one of SUB contiguous parts of
//                                the chunk; the threads of a wavefront are neighbouring rows of the same part, so the LDS reads
//                                are broadcasts.  Per record the item forms the window of the row's S0 <= 33 shifts along axis 0: a
//                                run of S0 bits of the volume's row (c_1, c_2), out of one or two u64 words, zero beyond either end
//                                of the row (the next bits in memory are the NEXT row's) and never shifted by 64.  The low 32 bits
//                                are added into VL_P bit planes by a ripple carry (plane p holds bit p of 32 counters), bit 32 into a
//                                counter of its own; after 2^VL_P - 1 records the planes are flushed into 33 u32 counters, and at the
//                                end every non-zero counter is added to hits by one relaxed atomicAdd.
//   voxel_locate_best_kernel   : one workgroup per candidate reduces the 64-bit maximum of hits << 32 | (0xFFFFFFFF - index): the
//                                largest score, and among equal scores the smallest index.
//
// §7c's conditions: relaxed device-scope atomics only, no fence, no waiting on another workgroup, scratch 0 (no array is indexed by a
// run-time value).  Bounds: a row's word index is tested against the row's words before every load; B < 2^30.
// The host logic (argument checks, candidates, ranking, selection and the loop) is host/voxel_locate.h.
#include "kernels.h"
#include "voxel_locate.h"

namespace {
typedef unsigned long long u64;
typedef long long i64;
constexpr int VL_T = VOXEL_THREADS;
constexpr int VL_OCC_T = VOXEL_OCCUPANCY_THREADS;
constexpr int VL_C = VOXEL_LOCATE_CHUNK;
constexpr int VL_P = 6;                      // bit planes: a flush every 63 records
constexpr int VL_FLUSH = (1 << VL_P) - 1;
constexpr int VL_NONE = -(1 << 30);          // the staged j_1 of a record no row accepts
constexpr u64 VL_EMPTY = ~0ull;

struct VoxelOccupancyArgs {
  const u64 *keys, *ci;
  u64 cap;
  unsigned min_count;
  int o[3], d[3];
  u64* bits;
  unsigned* counts;
};

__global__ __launch_bounds__(VL_OCC_T) void voxel_occupancy_kernel(VoxelOccupancyArgs a) {
  const size_t i = (size_t)blockIdx.x * VL_OCC_T + (size_t)threadIdx.x;
  bool inside = false, outside = false;
  if (i < a.cap) {
    const u64 key = a.keys[i];
    if (key != VL_EMPTY && (a.ci[i] >> 40) >= (u64)a.min_count) {
      int j[3];
      bool in = true;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        j[r] = (int)((key >> (21 * r)) & 0x1FFFFFull) - (1 << 20) - a.o[r];
        in = in && j[r] >= 0 && j[r] < a.d[r];
      }
      if (in) {
        const size_t B = (size_t)j[0] + (size_t)a.d[0] * ((size_t)j[1] + (size_t)a.d[1] * (size_t)j[2]);  // below 2^30
        __hip_atomic_fetch_or(&a.bits[B >> 6], 1ull << (B & 63), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      inside = in; outside = !in;
    }
  }
  // the two counts: a ballot per wavefront, an LDS add per wavefront, one atomicAdd per workgroup and non-zero count (every add
  // goes to the same two words: one per wavefront made the launch fifteen times as slow as the walk)
  __shared__ unsigned sC[2];
  if (threadIdx.x < 2) sC[threadIdx.x] = 0;
  __syncthreads();
  const u64 bi = __ballot(inside), bo = __ballot(outside);
  if ((threadIdx.x & 63) == 0) {
    if (bi) atomicAdd(&sC[0], (unsigned)__popcll(bi));
    if (bo) atomicAdd(&sC[1], (unsigned)__popcll(bo));
  }
  __syncthreads();
  if (threadIdx.x < 2 && sC[threadIdx.x]) __hip_atomic_fetch_add(&a.counts[threadIdx.x], sC[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct VoxelLocateArgs {
  const svo_cloud_point* pts;
  int n, k0;  // this launch's candidates are k0 + blockIdx.y
  float voxel_size, max_depth;
  int o[3], d[3], r[3];
  const u64* bits;
  unsigned* hits;
  svo_voxel_locate_best* best;
  double m[VOXEL_LOCATE_LAUNCH_K][12];
};

// Phase 1 of both forms: the chunk's j into LDS, n_used and n_inside into best[k].
__device__ __forceinline__ void vl_stage(const VoxelLocateArgs& a, int (*sj)[VL_C], unsigned* sN, int base, int cnt, int kk) {
  const int tid = threadIdx.x;
  const double* m = a.m[kk];
  const double vs = (double)a.voxel_size;
  if (tid < 2) sN[tid] = 0;
  __syncthreads();
  unsigned used = 0, inside = 0;
  for (int i = tid; i < VL_C; i += VL_T) {
    int j[3] = {0, VL_NONE, 0};
    if (i < cnt) {
      const svo_cloud_point p = a.pts[(size_t)base + (size_t)i];
      const float x = p.x, y = p.y, z = p.z;
      if (z > 0.0f && !(a.max_depth > 0.0f && z > a.max_depth) && fabsf(x) < VOXEL_ALIGN_MAX_ABS && fabsf(y) < VOXEL_ALIGN_MAX_ABS &&
          fabsf(z) < VOXEL_ALIGN_MAX_ABS) {
        const double P[3] = {(double)x, (double)y, (double)z};
        bool ok = true;
        double q[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          const double w = m[4 * r] * P[0] + m[4 * r + 1] * P[1] + m[4 * r + 2] * P[2] + m[4 * r + 3];
          q[r] = w / vs;
          ok = ok && q[r] >= -VOXEL_LOCATE_LIMIT && q[r] < VOXEL_LOCATE_LIMIT;
        }
        if (ok) {
          bool in = true, reach = true;
          int t[3];
#pragma unroll
          for (int r = 0; r < 3; ++r) {
            t[r] = (int)floor(q[r]) - a.o[r];
            in = in && t[r] >= 0 && t[r] < a.d[r];
            reach = reach && t[r] + a.r[r] >= 0 && t[r] - a.r[r] < a.d[r];
          }
          ++used;
          inside += in ? 1u : 0u;
          if (reach) { j[0] = t[0]; j[1] = t[1]; j[2] = t[2]; }
        }
      }
    }
    sj[0][i] = j[0]; sj[1][i] = j[1]; sj[2][i] = j[2];
  }
  if (used) atomicAdd(&sN[0], used);
  if (inside) atomicAdd(&sN[1], inside);
  __syncthreads();
  if (tid < 2 && sN[tid]) {
    unsigned* to = tid == 0 ? &a.best[a.k0 + kk].n_used : &a.best[a.k0 + kk].n_inside;
    __hip_atomic_fetch_add(to, sN[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

#ifndef SVO_EXP_LOCATE_BASELINE
__global__ __launch_bounds__(VL_T) void voxel_locate_scores_kernel(VoxelLocateArgs a) {
  __shared__ int sj[3][VL_C];
  __shared__ unsigned sN[2];
  const int tid = threadIdx.x, kk = blockIdx.y;
  const int base = (int)blockIdx.x * VL_C;
  const int cnt = a.n - base < VL_C ? a.n - base : VL_C;
  vl_stage(a, sj, sN, base, cnt, kk);
  const int r0 = a.r[0], r1 = a.r[1], r2 = a.r[2];
  const int S0 = 2 * r0 + 1, S1 = 2 * r1 + 1, S2 = 2 * r2 + 1, rows = S1 * S2;
  const int sub_n = rows >= 64 ? 4 : 64, per = VL_C / sub_n;  // few rows: more parts, so that the workgroup's threads have work
  const int items = rows * sub_n;
  const int wpr = a.d[0] >> 6;  // words per row of the volume
  const u64 wmask = (1ull << S0) - 1ull;
  unsigned* const hits = a.hits + (size_t)(a.k0 + kk) * (size_t)(S0 * rows);
  for (int it = tid; it < items; it += VL_T) {
    const int row = it % rows, sub = it / rows;
    const int s1 = row % S1 - r1, s2 = row / S1 - r2;
    const int begin = sub * per, end = cnt < begin + per ? cnt : begin + per;
    unsigned c[33];
#pragma unroll
    for (int b = 0; b < 33; ++b) c[b] = 0;
    for (int i0 = begin; i0 < end; i0 += VL_FLUSH) {
      const int e = end < i0 + VL_FLUSH ? end : i0 + VL_FLUSH;
      unsigned pl[VL_P];
#pragma unroll
      for (int p = 0; p < VL_P; ++p) pl[p] = 0;
#pragma unroll 4
      for (int i = i0; i < e; ++i) {
        const int c1 = sj[1][i] + s1, c2 = sj[2][i] + s2;
        const int lo = sj[0][i] - r0;          // bit t of the window is c_0 = lo + t
        const int wi = lo >> 6, off = lo & 63;  // arithmetic shift: a window that starts below the row has wi < 0
        // the ADDRESS is selected, not the load: a word outside the row, or a row outside the volume, reads word 0 of
        // a row that exists and is dropped, so that the loads of the unrolled records are all in flight before the first is used
        const bool row_ok = (unsigned)c1 < (unsigned)a.d[1] && (unsigned)c2 < (unsigned)a.d[2];
        const bool ok0 = row_ok && (unsigned)wi < (unsigned)wpr, ok1 = row_ok && off != 0 && (unsigned)(wi + 1) < (unsigned)wpr;
        const u64* rowp = a.bits + (size_t)wpr * (row_ok ? (size_t)c1 + (size_t)a.d[1] * (size_t)c2 : (size_t)0);
        u64 w0 = rowp[ok0 ? wi : 0], w1 = rowp[ok1 ? wi + 1 : 0];
        w0 = ok0 ? w0 : 0ull;
        w1 = ok1 ? w1 : 0ull;  // off == 0: the window is inside w0, and a shift by 64 is not made
        const u64 win = ((w0 >> off) | (w1 << ((64 - off) & 63))) & wmask;
        unsigned carry = (unsigned)win;
#pragma unroll
        for (int p = 0; p < VL_P; ++p) {
          const unsigned t = pl[p] & carry;
          pl[p] ^= carry;
          carry = t;
        }
        c[32] += (unsigned)(win >> 32);
      }
#pragma unroll
      for (int b = 0; b < 32; ++b) {
        unsigned v = 0;
#pragma unroll
        for (int p = 0; p < VL_P; ++p) v += (pl[p] >> b & 1u) << p;
        c[b] += v;
      }
    }
    unsigned* const to = hits + (size_t)((s2 + r2) * S1 + (s1 + r1)) * (size_t)S0;
#pragma unroll
    for (int b = 0; b < 33; ++b) {
      if (b < S0 && c[b]) __hip_atomic_fetch_add(&to[b], c[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}
#else
// The baseline form, built only for the measurement of DESIGN §7s: one thread per (record, row), one test per shift along axis 0 and
// one relaxed atomicAdd per hit, into LDS counters of the row block the workgroup works on.
__global__ __launch_bounds__(VL_T) void voxel_locate_scores_kernel(VoxelLocateArgs a) {
  __shared__ int sj[3][VL_C];
  __shared__ unsigned sN[2];
  __shared__ unsigned sH[64 * 33];
  const int tid = threadIdx.x, kk = blockIdx.y;
  const int base = (int)blockIdx.x * VL_C;
  const int cnt = a.n - base < VL_C ? a.n - base : VL_C;
  vl_stage(a, sj, sN, base, cnt, kk);
  const int r0 = a.r[0], r1 = a.r[1], r2 = a.r[2];
  const int S0 = 2 * r0 + 1, S1 = 2 * r1 + 1, S2 = 2 * r2 + 1, rows = S1 * S2;
  unsigned* const hits = a.hits + (size_t)(a.k0 + kk) * (size_t)(S0 * rows);
  for (int rb = 0; rb < rows; rb += 64) {  // a block of 64 rows at a time: 64 * 33 LDS counters
    const int nr = rows - rb < 64 ? rows - rb : 64;
    __syncthreads();
    for (int i = tid; i < nr * S0; i += VL_T) sH[i] = 0;
    __syncthreads();
    for (int it = tid; it < nr * cnt; it += VL_T) {
      const int rr = it % nr, i = it / nr, row = rb + rr;
      const int c1 = sj[1][i] + row % S1 - r1, c2 = sj[2][i] + row / S1 - r2;
      if ((unsigned)c1 >= (unsigned)a.d[1] || (unsigned)c2 >= (unsigned)a.d[2]) continue;
      const size_t rowbit = (size_t)a.d[0] * ((size_t)c1 + (size_t)a.d[1] * (size_t)c2);
      for (int t = 0; t < S0; ++t) {
        const int c0 = sj[0][i] - r0 + t;
        if ((unsigned)c0 >= (unsigned)a.d[0]) continue;
        const size_t B = rowbit + (size_t)c0;
        if (a.bits[B >> 6] >> (B & 63) & 1ull) atomicAdd(&sH[rr * S0 + t], 1u);
      }
    }
    __syncthreads();
    for (int i = tid; i < nr * S0; i += VL_T) {
      if (sH[i]) __hip_atomic_fetch_add(&hits[(size_t)rb * S0 + i], sH[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}
#endif

struct VoxelLocateBestArgs {
  const unsigned* hits;
  svo_voxel_locate_best* best;
  int S[3], r[3];
};

__global__ __launch_bounds__(VL_T) void voxel_locate_best_kernel(VoxelLocateBestArgs a) {
  const int tid = threadIdx.x, k = blockIdx.x;
  const int SS = a.S[0] * a.S[1] * a.S[2];
  const unsigned* h = a.hits + (size_t)k * (size_t)SS;
  u64 v = 0xFFFFFFFFull;  // score 0 at index 0: what all-zero scores give
  for (int i = tid; i < SS; i += VL_T) {
    const u64 t = (u64)h[i] << 32 | (u64)(0xFFFFFFFFu - (unsigned)i);
    v = t > v ? t : v;
  }
  for (int o = 32; o > 0; o >>= 1) {
    const u64 t = __shfl_xor(v, o);
    v = t > v ? t : v;
  }
  __shared__ u64 sV[VL_T / 64];
  if ((tid & 63) == 0) sV[tid >> 6] = v;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < VL_T / 64; ++w) v = sV[w] > v ? sV[w] : v;
    const unsigned index = 0xFFFFFFFFu - (unsigned)v;
    svo_voxel_locate_best* b = &a.best[k];  // n_used and n_inside are the score launch's
    b->hits_max = (unsigned)(v >> 32);
    b->s0 = (int)(index % (unsigned)a.S[0]) - a.r[0];
    b->s1 = (int)(index / (unsigned)a.S[0] % (unsigned)a.S[1]) - a.r[1];
    b->s2 = (int)(index / (unsigned)(a.S[0] * a.S[1])) - a.r[2];
    b->index = index;
    b->zero = 0;
  }
}
}  // namespace

// ----------------------------------------------------------------------------- host side
extern "C" int svo_voxel_occupancy_bytes(const int* dims3, size_t* bytes) { return voxel_occupancy_bytes(dims3, bytes); }
extern "C" int svo_voxel_locate_default_params(float voxel_size, svo_voxel_locate_params* params) { return voxel_locate_default_params(voxel_size, params); }
extern "C" int svo_voxel_locate_workspace_bytes(const svo_voxel_locate_params* params, size_t* bytes) { return voxel_locate_workspace_bytes(params, bytes); }

// The memsets and the launch of checked arguments.
static int voxel_occupancy_launch(const SvoVoxelView& t, int min_count, const int* origin, const int* dims, uint64_t* bits, uint32_t* counts) {
  svo_ctx* ctx = t.ctx;
  SvoProfScope prof(ctx, SVO_PROF_VOXEL_OCCUPANCY);
  SVO_HIP_CHECK(ctx, hipMemsetAsync(bits, 0, 8 * voxel_occupancy_words(dims), ctx->stream));
  SVO_HIP_CHECK(ctx, hipMemsetAsync(counts, 0, 2 * sizeof(uint32_t), ctx->stream));
  VoxelOccupancyArgs a{};
  a.keys = t.keys; a.ci = t.ci;
  a.cap = t.mask + 1;
  a.min_count = (unsigned)min_count;
  for (int r = 0; r < 3; ++r) { a.o[r] = origin[r]; a.d[r] = dims[r]; }
  a.bits = reinterpret_cast<u64*>(bits);
  a.counts = counts;
  hipLaunchKernelGGL(voxel_occupancy_kernel, dim3((unsigned)voxel_occupancy_groups((size_t)a.cap)), dim3(VL_OCC_T), 0, ctx->stream, a);
  SVO_HIP_CHECK(ctx, hipGetLastError());
  return SVO_OK;
}

extern "C" int svo_voxel_map_occupancy_dev(svo_voxel_map* m, int min_count, const int* origin3, const int* dims3, uint64_t* bits, uint32_t* counts) {
  if (!m) return SVO_ERR_INVALID;
  const SvoVoxelView t = svo_voxel_map_view(m);
  svo_use_device(t.ctx);
  SVO_ARGS_CHECK(t.ctx, voxel_occupancy_check(min_count, origin3, dims3, bits, counts, true, &err));
  return voxel_occupancy_launch(t, min_count, origin3, dims3, bits, counts);
}

extern "C" int svo_voxel_map_occupancy(svo_voxel_map* m, int min_count, const int* origin3, const int* dims3, uint64_t* host_bits,
                                       uint32_t* host_counts) {
  if (!m) return SVO_ERR_INVALID;
  const SvoVoxelView t = svo_voxel_map_view(m);
  svo_ctx* ctx = t.ctx;
  svo_use_device(ctx);
  SVO_ARGS_CHECK(ctx, voxel_occupancy_check(min_count, origin3, dims3, host_bits, host_counts, false, &err));
  const size_t bytes = 8 * voxel_occupancy_words(dims3);
  SvoParts parts;
  const size_t o_bits = parts.add(bytes), o_counts = parts.add(2 * sizeof(uint32_t));
  SvoTemp d;
  SVO_HIP_CHECK(ctx, hipMalloc(&d.p, parts.total()));
  uint32_t c[2] = {0, 0};
  const int rc = svo_host_call(
      ctx, "voxel_map_occupancy", hipSuccess,
      [&] { return voxel_occupancy_launch(t, min_count, origin3, dims3, d.at<uint64_t>(o_bits), d.at<uint32_t>(o_counts)); },
      [&] {
        hipError_t e = hipMemcpyAsync(host_bits, d.at(o_bits), bytes, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess && host_counts) e = hipMemcpyAsync(c, d.at(o_counts), sizeof(c), hipMemcpyDeviceToHost, ctx->stream);
        return e;
      });
  if (rc) return rc;
  if (host_counts) memcpy(host_counts, c, sizeof(c));
  return SVO_OK;
}

// The memsets and the launches of checked arguments.
static int voxel_locate_launch(const SvoVoxelView& t, const uint64_t* bits, const int* origin, const int* dims, const svo_cloud_point* points, int n,
                               const double* mats, int K, const int* box, uint32_t* hits, svo_voxel_locate_best* best) {
  svo_ctx* ctx = t.ctx;
  SvoProfScope prof(ctx, SVO_PROF_VOXEL_LOCATE);
  SVO_HIP_CHECK(ctx, hipMemsetAsync(hits, 0, sizeof(uint32_t) * (size_t)K * voxel_locate_shifts(box), ctx->stream));
  SVO_HIP_CHECK(ctx, hipMemsetAsync(best, 0, sizeof(svo_voxel_locate_best) * (size_t)K, ctx->stream));
  for (int k0 = 0; n > 0 && k0 < K; k0 += VOXEL_LOCATE_LAUNCH_K) {
    const int nk = K - k0 < VOXEL_LOCATE_LAUNCH_K ? K - k0 : VOXEL_LOCATE_LAUNCH_K;
    VoxelLocateArgs a{};
    a.pts = points; a.n = n; a.k0 = k0;
    a.voxel_size = t.voxel_size; a.max_depth = t.max_depth;
    for (int r = 0; r < 3; ++r) { a.o[r] = origin[r]; a.d[r] = dims[r]; a.r[r] = box[r]; }
    a.bits = reinterpret_cast<const u64*>(bits);
    a.hits = hits; a.best = best;
    memcpy(a.m, mats + 12 * (size_t)k0, sizeof(double) * 12 * (size_t)nk);
    hipLaunchKernelGGL(voxel_locate_scores_kernel, dim3((unsigned)voxel_locate_chunks(n), (unsigned)nk), dim3(VL_T), 0, ctx->stream, a);
    SVO_HIP_CHECK(ctx, hipGetLastError());
  }
  VoxelLocateBestArgs b{};
  b.hits = hits; b.best = best;
  for (int r = 0; r < 3; ++r) { b.S[r] = 2 * box[r] + 1; b.r[r] = box[r]; }
  hipLaunchKernelGGL(voxel_locate_best_kernel, dim3((unsigned)K), dim3(VL_T), 0, ctx->stream, b);
  SVO_HIP_CHECK(ctx, hipGetLastError());
  return SVO_OK;
}

extern "C" int svo_voxel_map_locate_scores_dev(svo_voxel_map* m, const uint64_t* bits, const int* origin3, const int* dims3,
                                               const svo_cloud_point* points, int n, const double* mats, int K, const int* box3, uint32_t* hits,
                                               svo_voxel_locate_best* best) {
  if (!m) return SVO_ERR_INVALID;
  const SvoVoxelView t = svo_voxel_map_view(m);
  svo_use_device(t.ctx);
  SVO_ARGS_CHECK(t.ctx, voxel_locate_scores_check(bits, origin3, dims3, points, n, mats, K, box3, hits, best, &err));
  return voxel_locate_launch(t, bits, origin3, dims3, points, n, mats, K, box3, hits, best);
}

extern "C" int svo_voxel_map_locate(svo_voxel_map* m, const svo_voxel_normal* normals, const svo_cloud_point* points, int n, const double* pose7_in,
                                    const svo_voxel_locate_params* prm, const svo_voxel_align_params* aprm, void* workspace, double* pose7_out,
                                    svo_voxel_locate_result* result) {
  if (!m) return SVO_ERR_INVALID;
  const SvoVoxelView t = svo_voxel_map_view(m);
  svo_ctx* ctx = t.ctx;
  svo_use_device(ctx);
  SVO_ARGS_CHECK(ctx, voxel_locate_loop_check(normals, points, n, pose7_in, prm, aprm, workspace, pose7_out, result, &err));
  const VoxelLocateLayout l = voxel_locate_layout(prm);
  char* ws = static_cast<char*>(workspace);
  uint64_t* bits = reinterpret_cast<uint64_t*>(ws + l.bits);
  uint32_t *counts = reinterpret_cast<uint32_t*>(ws + l.counts), *hits = reinterpret_cast<uint32_t*>(ws + l.hits);
  svo_voxel_locate_best* best = reinterpret_cast<svo_voxel_locate_best*>(ws + l.best);
  const char* err = nullptr;
  const int rc = voxel_locate_loop(
      pose7_in, prm, t.voxel_size,
      [&](const double* mats, int K, const int* origin, svo_voxel_locate_best* host_best) {
        return svo_host_call(
            ctx, "voxel_map_locate", hipSuccess,
            [&] {
              const int rc = voxel_occupancy_launch(t, prm->min_count, origin, prm->dims, bits, counts);
              return rc ? rc : voxel_locate_launch(t, bits, origin, prm->dims, points, n, mats, K, prm->box, hits, best);
            },
            [&] { return hipMemcpyAsync(host_best, best, sizeof(svo_voxel_locate_best) * (size_t)K, hipMemcpyDeviceToHost, ctx->stream); });
      },
      [&](const double* pose7, double* out, svo_voxel_align_result* res) {
        return normals ? svo_voxel_map_align_plane(m, normals, points, n, pose7, aprm, out, res) : svo_voxel_map_align(m, points, n, pose7, aprm, out, res);
      },
      pose7_out, result, &err);
  if (rc == SVO_ERR_INVALID && err) ctx->err = err;
  return rc;
}
