// Voxel map align, plane form (include/svo.h, "Voxel map align, plane form"): every record of a cloud is matched with the
// nearest voxel mean among the 1 or 27 voxels around it exactly as csrc/voxel_align.hip matches it, and the normal equations of a
// point-to-plane pose increment along the matched voxel's normal are reduced to 28 integers.
//
//   voxel_align_plane_kernel<NC> : one thread per record, 256-thread workgroups, NC = 1 (reach 0) or 27 (reach 1) candidates.  The
//                          look-up is csrc/voxel_align.hip's, phase by phase (A the NC home slots' keys in one run of loads, B found /
//                          foreign as two bit masks, C the counts and D the sums with the ADDRESS selected, nine candidates at a
//                          time, E the rare probe continuation over the foreign mask).  What differs:
//                            - the running nearest match carries its slot as the 32-bit byte offset the look-up already has;
//                            - once the minimum is settled, ONE 16-byte load of normals[slot]: one more dependent round trip per
//                              record, not 27;
//                            - a match's 28 terms are host/voxel_align_plane.h's (the text a CPU program runs too), and 33 different
//                              words, not 20, go through the __shfl_xor tree, one LDS row per wavefront and one relaxed atomicAdd
//                              per workgroup and non-zero word.
//                          No array is indexed by a run-time value (scratch 0).  A thread without a contribution adds zeros and stays
//                          to the end: the shuffles are the whole wavefront's.
//
// §7c's conditions: relaxed device-scope atomics only, no fence, no waiting on another workgroup, scratch 0.  The launch claims
// nothing and writes nothing but the caller's 40 words.  csrc/voxel_align.hip is untouched: the look-up is restated here rather than
// moved into a shared header, so the two point-form instantiations compile to what they did.
#include "kernels.h"
#include "voxel_align_plane.h"

namespace {
typedef unsigned long long u64;
typedef long long i64;
constexpr int VP_T = VOXEL_THREADS;
constexpr u64 VP_EMPTY = ~0ull;
constexpr int VP_TERMS = VOXEL_ALIGN_PLANE_TERMS;
constexpr int VP_WORDS = VP_TERMS + 5;  // the different words of a launch: the 28 terms, then the five counts (word 0 is n_matched again)

struct VoxelAlignPlaneArgs {
  const svo_cloud_point* pts;
  int n;
  double m[12];
  float voxel_size, max_depth;
  const u64 *keys, *ci, *sx, *sy, *sz;
  const svo_voxel_normal* normals;
  u64 mask;
  unsigned min_count;
  double max_d2;
  u64* sums;  // 40 words, zeroed on the stream before the launch
};

__device__ __forceinline__ u64 vp_fmix64(u64 k) {  // the voxel map's hash (include/svo.h, "voxel map": Table)
  k ^= k >> 33; k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return k;
}

// The word at byte offset `off` of one of the table's arrays: a slot index is below 2^28, so its byte offset fits 32 bits.
__device__ __forceinline__ u64 vp_at(const u64* base, unsigned off) { return *reinterpret_cast<const u64*>(reinterpret_cast<const char*>(base) + off); }
__device__ __forceinline__ unsigned vp_hi(const u64* base, unsigned off) { return *reinterpret_cast<const unsigned*>(reinterpret_cast<const char*>(base) + off + 4u); }

template <int NC>
__device__ __forceinline__ u64 vp_key(u64 base, int c) {
  if (NC == 1) return base;
  const i64 i = c % 3 - 1, j = c / 3 % 3 - 1, l = c / 9 - 1;
  return (u64)((i64)base + i + j * (1ll << 21) + l * (1ll << 42));
}

// The running nearest match: smallest d2, among equal d2 the smallest key; off is its slot's byte offset in the table's arrays.
struct VpBest {
  double d2, e[3];
  u64 key;
  unsigned off;
  bool have;
};

__device__ __forceinline__ void vp_weigh(VpBest& b, u64 key, unsigned off, u64 count, u64 sx, u64 sy, u64 sz, const double (&w)[3], double vs) {
  const double c = (double)count * 65536.0;
  const u64 s[3] = {sx, sy, sz};
  double e[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double k = (double)((i64)((key >> (21 * r)) & 0x1FFFFFull) - (1ll << 20));
    e[r] = w[r] - (k + (double)s[r] / c) * vs;
  }
  const double d2 = e[0] * e[0] + e[1] * e[1] + e[2] * e[2];
  if (!b.have || d2 < b.d2 || (d2 == b.d2 && key < b.key)) {
    b.have = true; b.d2 = d2; b.key = key; b.off = off;
    b.e[0] = e[0]; b.e[1] = e[1]; b.e[2] = e[2];
  }
}

template <int NC>
__global__ __launch_bounds__(VP_T) void voxel_align_plane_kernel(VoxelAlignPlaneArgs a) {
  constexpr int G = NC == 1 ? 1 : 9;  // candidates per batch of phase D
  const int tid = threadIdx.x;
  const size_t i = (size_t)blockIdx.x * VP_T + (size_t)tid;
  const bool valid = i < (size_t)a.n;
  const double vs = (double)a.voxel_size;
  bool ok = false;
  double P[3] = {0.0, 0.0, 0.0}, w[3] = {0.0, 0.0, 0.0};
  u64 base = 0;
  if (valid) {
    const svo_cloud_point p = a.pts[i];  // one 16-byte load
    const float x = p.x, y = p.y, z = p.z;
    if (z > 0.0f && !(a.max_depth > 0.0f && z > a.max_depth) && fabsf(x) < VOXEL_ALIGN_MAX_ABS && fabsf(y) < VOXEL_ALIGN_MAX_ABS &&
        fabsf(z) < VOXEL_ALIGN_MAX_ABS) {
      P[0] = (double)x; P[1] = (double)y; P[2] = (double)z;
      bool in = true;
      double q[3];
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        w[r] = a.m[4 * r] * P[0] + a.m[4 * r + 1] * P[1] + a.m[4 * r + 2] * P[2] + a.m[4 * r + 3];
        q[r] = w[r] / vs;
        in = in && q[r] >= -VOXEL_ALIGN_LIMIT && q[r] < VOXEL_ALIGN_LIMIT;
      }
      if (in) {
        ok = true;
#pragma unroll
        for (int r = 0; r < 3; ++r) base |= (u64)((i64)floor(q[r]) + (1ll << 20)) << (21 * r);
      }
    }
  }
  VpBest best;
  best.have = false; best.d2 = 0.0; best.key = VP_EMPTY; best.off = 0u;
  best.e[0] = 0.0; best.e[1] = 0.0; best.e[2] = 0.0;
  if (ok) {
    // A: every home slot's key, asked for before any is waited for
    unsigned h[NC];  // the slot's BYTE offset in each of the five arrays: below 2^31
    u64 got[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) h[c] = (unsigned)(vp_fmix64(vp_key<NC>(base, c)) & a.mask) << 3;
#pragma unroll
    for (int c = 0; c < NC; ++c) got[c] = vp_at(a.keys, h[c]);
    // B: found at home / foreign at home (the keys are formed again from a copy of base the compiler cannot see through)
    unsigned found = 0, foreign = 0;
    u64 base_b = base;
    asm volatile("" : "+v"(base_b));
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const u64 key = vp_key<NC>(base_b, c);
      found |= got[c] == key ? 1u << c : 0u;
      foreign |= got[c] != key && got[c] != VP_EMPTY ? 1u << c : 0u;
    }
    // C: the counts of the slots found at home, all in flight: the address is selected, not the load
    constexpr int CENTRE = NC / 2;
    unsigned count[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) count[c] = vp_hi(a.ci, found >> c & 1u ? h[c] : h[CENTRE]);
#pragma unroll
    for (int c = 0; c < NC; ++c) count[c] = found >> c & 1u ? count[c] >> 8 : 0u;  // the count is bits 40..63; carved: 0
    // D: the sums of the qualifying slots by the same selection, G candidates at a time, then their distances
#pragma unroll
    for (int g0 = 0; g0 < NC; g0 += G) {
      u64 base_d = base;
      asm volatile("" : "+v"(base_d));
      u64 s[G][3];
#pragma unroll
      for (int c = 0; c < G; ++c) {
        const unsigned at = count[g0 + c] >= a.min_count ? h[g0 + c] : h[CENTRE];
        s[c][0] = vp_at(a.sx, at); s[c][1] = vp_at(a.sy, at); s[c][2] = vp_at(a.sz, at);
      }
#pragma unroll
      for (int c = 0; c < G; ++c) {
        if (count[g0 + c] >= a.min_count)
          vp_weigh(best, vp_key<NC>(base_d, g0 + c), h[g0 + c], (u64)count[g0 + c], s[c][0], s[c][1], s[c][2], w, vs);
      }
    }
    // E: the rare continuation: candidates whose home slot holds another key
    while (foreign) {
      const int c = __builtin_ctz(foreign);
      foreign &= foreign - 1u;
      const u64 key = vp_key<NC>(base, c);
      u64 at = vp_fmix64(key) & a.mask;
      for (int p = 1; p < SVO_VOXEL_MAX_PROBES; ++p) {  // the home slot was probe 0
        at = (at + 1ull) & a.mask;
        const u64 k = a.keys[at];
        if (k == VP_EMPTY) break;
        if (k == key) {
          const u64 count = a.ci[at] >> 40;
          if (count >= (u64)a.min_count) vp_weigh(best, key, (unsigned)at << 3, count, a.sx[at], a.sy[at], a.sz[at], w, vs);
          break;
        }
      }
    }
  }
  // the record's verdict, the matched voxel's normal (16 bytes per slot: twice the table's byte offset) and the terms
  const bool matched = ok && best.have && !(best.d2 > a.max_d2);
  double nn[3] = {0.0, 0.0, 0.0};
  if (matched) {
    const float4 f = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(a.normals) + ((size_t)best.off << 1));
    nn[0] = (double)f.x; nn[1] = (double)f.y; nn[2] = (double)f.z;
  }
  const bool contributes = matched && !(nn[0] == 0.0 && nn[1] == 0.0 && nn[2] == 0.0);
  i64 v[VP_WORDS];
#pragma unroll
  for (int k = 0; k < VP_WORDS; ++k) v[k] = 0;
  if (contributes) voxel_align_plane_terms(nn, best.e, a.m, P, v);
  v[VP_TERMS] = contributes ? 1 : 0;
  v[VP_TERMS + 1] = valid && !ok ? 1 : 0;
  v[VP_TERMS + 2] = ok && !best.have ? 1 : 0;
  v[VP_TERMS + 3] = ok && best.have && !matched ? 1 : 0;
  v[VP_TERMS + 4] = matched && !contributes ? 1 : 0;
  // wavefront tree, one LDS row per wavefront, one atomicAdd per workgroup and non-zero word
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int k = 0; k < VP_WORDS; ++k) v[k] += __shfl_xor(v[k], o);
  }
  __shared__ i64 sW[VP_T / 64][VP_WORDS];
  if ((tid & 63) == 0) {
#pragma unroll
    for (int k = 0; k < VP_WORDS; ++k) sW[tid >> 6][k] = v[k];
  }
  __syncthreads();
  if (tid <= VP_WORDS) {  // word 0 is n_matched again; word t > 0 is v[t - 1]
    const int k = tid == 0 ? VP_TERMS : tid - 1;
    i64 t = 0;
    for (int wv = 0; wv < VP_T / 64; ++wv) t += sW[wv][k];
    if (t) __hip_atomic_fetch_add(&a.sums[tid], (u64)t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}
}  // namespace

// ----------------------------------------------------------------------------- host side
// The memset and the launch of checked arguments.
static int voxel_align_plane_launch(const SvoVoxelView& t, const svo_voxel_normal* normals, const svo_cloud_point* points, int n, const double* c2w12,
                                    const svo_voxel_align_params* prm, int64_t* sums) {
  svo_ctx* ctx = t.ctx;
  SvoProfScope prof(ctx, SVO_PROF_VOXEL_ALIGN_PLANE);
  SVO_HIP_CHECK(ctx, hipMemsetAsync(sums, 0, VOXEL_ALIGN_PLANE_WORDS * sizeof(int64_t), ctx->stream));
  if (n == 0) return SVO_OK;
  VoxelAlignPlaneArgs a{};
  a.pts = points; a.n = n;
  memcpy(a.m, c2w12, sizeof(a.m));
  a.voxel_size = t.voxel_size; a.max_depth = t.max_depth;
  a.keys = t.keys; a.ci = t.ci; a.sx = t.sx; a.sy = t.sy; a.sz = t.sz;
  a.normals = normals;
  a.mask = t.mask;
  a.min_count = (unsigned)prm->min_count;
  a.max_d2 = (double)prm->max_dist * (double)prm->max_dist;
  a.sums = reinterpret_cast<u64*>(sums);
  const dim3 grid((unsigned)voxel_align_groups(n)), block(VP_T);
  if (prm->reach == 0) hipLaunchKernelGGL(voxel_align_plane_kernel<1>, grid, block, 0, ctx->stream, a);
  else hipLaunchKernelGGL(voxel_align_plane_kernel<27>, grid, block, 0, ctx->stream, a);
  SVO_HIP_CHECK(ctx, hipGetLastError());
  return SVO_OK;
}

extern "C" int svo_voxel_map_align_plane_sums_dev(svo_voxel_map* m, const svo_voxel_normal* normals, const svo_cloud_point* points, int n,
                                                  const double* c2w12, const svo_voxel_align_params* prm, int64_t* sums) {
  if (!m) return SVO_ERR_INVALID;
  const SvoVoxelView t = svo_voxel_map_view(m);
  svo_use_device(t.ctx);
  SVO_ARGS_CHECK(t.ctx, voxel_align_plane_sums_check(normals, points, n, c2w12, prm, sums, &err));
  return voxel_align_plane_launch(t, normals, points, n, c2w12, prm, sums);
}

extern "C" int svo_voxel_map_align_plane_sums_pose7_dev(svo_voxel_map* m, const svo_voxel_normal* normals, const svo_cloud_point* points, int n,
                                                        const double* pose7, const svo_voxel_align_params* prm, int64_t* sums) {
  if (!m) return SVO_ERR_INVALID;
  svo_ctx* ctx = svo_voxel_map_view(m).ctx;
  SVO_ARGS_CHECK(ctx, voxel_align_plane_normals_check(normals, &err));
  SVO_ARGS_CHECK(ctx, voxel_align_n_check(n, &err));
  SVO_REQUIRE(ctx, pose7, "voxel_map_align_plane: null pose7");
  double m12[12];
  voxel_pose7_to_cam_to_world(pose7, m12);
  return svo_voxel_map_align_plane_sums_dev(m, normals, points, n, m12, prm, sums);
}

extern "C" int svo_voxel_map_align_plane(svo_voxel_map* m, const svo_voxel_normal* normals, const svo_cloud_point* points, int n,
                                         const double* pose7_in, const svo_voxel_align_params* prm, double* pose7_out,
                                         svo_voxel_align_result* result) {
  if (!m) return SVO_ERR_INVALID;
  const SvoVoxelView t = svo_voxel_map_view(m);
  svo_ctx* ctx = t.ctx;
  svo_use_device(ctx);
  SVO_ARGS_CHECK(ctx, voxel_align_plane_loop_check(normals, points, n, pose7_in, prm, pose7_out, result, &err));
  SvoScratch scratch(ctx);
  int64_t* d = scratch.take<int64_t>(VOXEL_ALIGN_PLANE_WORDS);  // the context's scratch: every iteration ends with the stream drained
  SVO_REQUIRE(ctx, d, "voxel_map_align_plane: the context has no scratch");
  return voxel_align_plane_loop(
      pose7_in, prm,
      [&](const double* m12, int64_t* w) {
        return svo_host_call(
            ctx, "voxel_map_align_plane", hipSuccess, [&] { return voxel_align_plane_launch(t, normals, points, n, m12, prm, d); },
            [&] { return hipMemcpyAsync(w, d, VOXEL_ALIGN_PLANE_WORDS * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream); });
      },
      pose7_out, result);
}
