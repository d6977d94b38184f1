// Voxel map align (include/svo.h, "Voxel map align"): every record of a cloud is matched with the nearest voxel mean
// among the 1 or 27 voxels around it, and the normal equations of a point-to-point pose increment are reduced to 21 integers.
//
//   voxel_align_kernel<NC> : one thread per record, 256-thread workgroups, NC = 1 (reach 0) or 27 (reach 1) candidates.  The hot part
//                          is NC look-ups per record at unrelated table addresses, so the look-up is written in phases, each a fully
//                          unrolled loop over the candidates with nothing but independent loads in it:
//                            A  the candidates' keys, their home slots, and ALL NC home-slot key loads;
//                            B  found / foreign per candidate from the loaded keys (two bit masks);
//                            C  the count | intensity words, all in flight: the ADDRESS is selected, not the load (a candidate
//                               that was not found reads the centre candidate's home slot again and its word is dropped), because
//                               a load under a branch was waited for inside the branch, one candidate after the other;
//                            D  the three sum words of the qualifying slots by the same selection, nine candidates at a time (54
//                               registers of loads in flight instead of 162), then their distances;
//                            E  the rare probe continuation: a loop over the set bits of the foreign mask that recomputes the
//                               candidate's key from its number and walks on by plain loads (the removal's rule: EMPTY is absent,
//                               64 slots at the most); a candidate found there is weighed at once, since the nearest match is a
//                               minimum and a minimum takes its arguments in any order.
//                          No array is indexed by a run-time value (scratch 0).  A thread without a match contributes zeros and
//                          stays to the end: the shuffles are the whole wavefront's.  The 20 different words go through a
//                          __shfl_xor tree on the 64-bit integers, one LDS row per wavefront, and one relaxed atomicAdd per
//                          workgroup and non-zero word.
//
// §7c's conditions: relaxed device-scope atomics only, no fence, no waiting on another workgroup, scratch 0; offsets are 64-bit except a
// slot's byte offset inside one array, which is below 2^31 (va_at).  The
// launch claims nothing and writes nothing but the caller's 32 words: every key it reads was written by an earlier launch on the
// same stream, so a load decides (csrc/voxel.hip, vx_find).
// The host logic (argument checks, Q_S, the 6 x 6 solve, the pose update and the loop) is host/voxel_align.h.
#include "kernels.h"
#include "voxel_align.h"

namespace {
typedef unsigned long long u64;
typedef long long i64;
constexpr int VA_T = VOXEL_THREADS;
constexpr u64 VA_EMPTY = ~0ull;
constexpr int VA_WORDS = 20;  // the different words of a launch: 1..16, then the four counts (word 0 is n_matched again)

struct VoxelAlignArgs {
  const svo_cloud_point* pts;
  int n;
  double m[12];
  float voxel_size, max_depth;
  const u64 *keys, *ci, *sx, *sy, *sz;
  u64 mask;
  unsigned min_count;
  double max_d2;
  u64* sums;  // 32 words, zeroed on the stream before the launch
};

__device__ __forceinline__ u64 va_fmix64(u64 k) {  // the voxel map's hash (include/svo.h, "voxel map": Table)
  k ^= k >> 33; k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return k;
}

// The word at byte offset `off` of one of the table's arrays.  A slot index is below 2^28 (capacity_log2 <= 28), so its byte offset fits
// 32 bits and the load takes the array's base from scalar registers: one address register per load in flight instead of two.
__device__ __forceinline__ u64 va_at(const u64* base, unsigned off) { return *reinterpret_cast<const u64*>(reinterpret_cast<const char*>(base) + off); }

// The high half of that word: of a count | intensity word it holds the count in its bits 8..31.
__device__ __forceinline__ unsigned va_hi(const u64* base, unsigned off) { return *reinterpret_cast<const unsigned*>(reinterpret_cast<const char*>(base) + off + 4u); }

// Candidate c of NC: the key of k + (i, j, l), (i, j, l) = (c % 3 - 1, c / 3 % 3 - 1, c / 9 - 1) for NC == 27, k itself for NC == 1.
// base is the key of k; no index leaves its 21 bits (rule 1), so the offsets add without a carry between the fields.
template <int NC>
__device__ __forceinline__ u64 va_key(u64 base, int c) {
  if (NC == 1) return base;
  const i64 i = c % 3 - 1, j = c / 3 % 3 - 1, l = c / 9 - 1;
  return (u64)((i64)base + i + j * (1ll << 21) + l * (1ll << 42));
}

// The running nearest match: smallest d2, among equal d2 the smallest key.
struct VaBest {
  double d2, e[3];
  u64 key;
  bool have;
};

__device__ __forceinline__ void va_weigh(VaBest& b, u64 key, u64 count, u64 sx, u64 sy, u64 sz, const double (&w)[3], double vs) {
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
    b.have = true; b.d2 = d2; b.key = key;
    b.e[0] = e[0]; b.e[1] = e[1]; b.e[2] = e[2];
  }
}

template <int NC>
__global__ __launch_bounds__(VA_T) void voxel_align_kernel(VoxelAlignArgs a) {
  constexpr int G = NC == 1 ? 1 : 9;  // candidates per batch of phase D
  const int tid = threadIdx.x;
  const size_t i = (size_t)blockIdx.x * VA_T + (size_t)tid;
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
  VaBest best;
  best.have = false; best.d2 = 0.0; best.key = VA_EMPTY;
  best.e[0] = 0.0; best.e[1] = 0.0; best.e[2] = 0.0;
  if (ok) {
    // A: every home slot's key, asked for before any is waited for (a slot index fits 32 bits: capacity_log2 <= 28)
    unsigned h[NC];  // the slot's BYTE offset in each of the five arrays: below 2^31
    u64 got[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) h[c] = (unsigned)(va_fmix64(va_key<NC>(base, c)) & a.mask) << 3;
#pragma unroll
    for (int c = 0; c < NC; ++c) got[c] = va_at(a.keys, h[c]);
    // B: found at home / foreign at home
    // (the 27 keys are formed again from a copy of base the compiler cannot see through, here and in D: kept from phase A they
    // held 54 registers to the end and the kernel ran at one wavefront per SIMD; the empty statement emits no instruction)
    unsigned found = 0, foreign = 0;
    u64 base_b = base;
    asm volatile("" : "+v"(base_b));
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const u64 key = va_key<NC>(base_b, c);
      found |= got[c] == key ? 1u << c : 0u;
      foreign |= got[c] != key && got[c] != VA_EMPTY ? 1u << c : 0u;
    }
    // C: the counts of the slots found at home (the high half of the count | intensity word), all in flight.  A load under a
    // branch was waited for inside the branch, one candidate after the other; so the address is selected instead and
    // every candidate loads: one that was not found reads the centre candidate's home slot again, a line that is on its way
    // anyway, and its word is dropped.
    constexpr int CENTRE = NC / 2;
    unsigned count[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) count[c] = va_hi(a.ci, found >> c & 1u ? h[c] : h[CENTRE]);
#pragma unroll
    for (int c = 0; c < NC; ++c) count[c] = found >> c & 1u ? count[c] >> 8 : 0u;  // the count is bits 40..63; carved: 0
    // D: the sums of the qualifying slots by the same selection, G candidates at a time, then their distances (min_count >= 1: a
    // slot that was not found, or a carved one, has count 0 and does not qualify)
#pragma unroll
    for (int g0 = 0; g0 < NC; g0 += G) {
      u64 base_d = base;
      asm volatile("" : "+v"(base_d));
      u64 s[G][3];
#pragma unroll
      for (int c = 0; c < G; ++c) {
        const unsigned at = count[g0 + c] >= a.min_count ? h[g0 + c] : h[CENTRE];
        s[c][0] = va_at(a.sx, at); s[c][1] = va_at(a.sy, at); s[c][2] = va_at(a.sz, at);
      }
#pragma unroll
      for (int c = 0; c < G; ++c) {
        if (count[g0 + c] >= a.min_count) va_weigh(best, va_key<NC>(base_d, g0 + c), (u64)count[g0 + c], s[c][0], s[c][1], s[c][2], w, vs);
      }
    }
    // E: the rare continuation: candidates whose home slot holds another key
    while (foreign) {
      const int c = __builtin_ctz(foreign);
      foreign &= foreign - 1u;
      const u64 key = va_key<NC>(base, c);
      u64 at = va_fmix64(key) & a.mask;
      for (int p = 1; p < SVO_VOXEL_MAX_PROBES; ++p) {  // the home slot was probe 0
        at = (at + 1ull) & a.mask;
        const u64 k = a.keys[at];
        if (k == VA_EMPTY) break;
        if (k == key) {
          const u64 count = a.ci[at] >> 40;
          if (count >= (u64)a.min_count) va_weigh(best, key, count, a.sx[at], a.sy[at], a.sz[at], w, vs);
          break;
        }
      }
    }
  }
  // the record's verdict and its terms (zeros unless matched)
  const bool matched = ok && best.have && !(best.d2 > a.max_d2);
  i64 v[VA_WORDS];
#pragma unroll
  for (int k = 0; k < VA_WORDS; ++k) v[k] = 0;
  if (matched) {
    double c[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) c[r] = a.m[r] * best.e[0] + a.m[4 + r] * best.e[1] + a.m[8 + r] * best.e[2];
    v[0] = voxel_align_q(P[0], VOXEL_ALIGN_S16); v[1] = voxel_align_q(P[1], VOXEL_ALIGN_S16); v[2] = voxel_align_q(P[2], VOXEL_ALIGN_S16);
    v[3] = voxel_align_q(P[0] * P[0], VOXEL_ALIGN_S16); v[4] = voxel_align_q(P[0] * P[1], VOXEL_ALIGN_S16);
    v[5] = voxel_align_q(P[0] * P[2], VOXEL_ALIGN_S16); v[6] = voxel_align_q(P[1] * P[1], VOXEL_ALIGN_S16);
    v[7] = voxel_align_q(P[1] * P[2], VOXEL_ALIGN_S16); v[8] = voxel_align_q(P[2] * P[2], VOXEL_ALIGN_S16);
    v[9] = voxel_align_q(c[0], VOXEL_ALIGN_S28); v[10] = voxel_align_q(c[1], VOXEL_ALIGN_S28); v[11] = voxel_align_q(c[2], VOXEL_ALIGN_S28);
    v[12] = voxel_align_q(P[1] * c[2] - P[2] * c[1], VOXEL_ALIGN_S28);
    v[13] = voxel_align_q(P[2] * c[0] - P[0] * c[2], VOXEL_ALIGN_S28);
    v[14] = voxel_align_q(P[0] * c[1] - P[1] * c[0], VOXEL_ALIGN_S28);
    v[15] = voxel_align_q(c[0] * c[0] + c[1] * c[1] + c[2] * c[2], VOXEL_ALIGN_S28);
  }
  v[16] = matched ? 1 : 0;
  v[17] = valid && !ok ? 1 : 0;
  v[18] = ok && !best.have ? 1 : 0;
  v[19] = ok && best.have && !matched ? 1 : 0;
  // wavefront tree, one LDS row per wavefront, one atomicAdd per workgroup and non-zero word
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int k = 0; k < VA_WORDS; ++k) v[k] += __shfl_xor(v[k], o);
  }
  __shared__ i64 sW[VA_T / 64][VA_WORDS];
  if ((tid & 63) == 0) {
#pragma unroll
    for (int k = 0; k < VA_WORDS; ++k) sW[tid >> 6][k] = v[k];
  }
  __syncthreads();
  if (tid <= VA_WORDS) {  // word 0 is n_matched again; word t > 0 is v[t - 1]
    const int k = tid == 0 ? 16 : tid - 1;
    i64 t = 0;
    for (int wv = 0; wv < VA_T / 64; ++wv) t += sW[wv][k];
    if (t) __hip_atomic_fetch_add(&a.sums[tid], (u64)t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}
}  // namespace

// ----------------------------------------------------------------------------- host side
extern "C" int svo_voxel_align_default_params(float voxel_size, svo_voxel_align_params* params) { return voxel_align_default_params(voxel_size, params); }

// The memset and the launch of checked arguments.
static int voxel_align_launch(const SvoVoxelView& t, const svo_cloud_point* points, int n, const double* c2w12, const svo_voxel_align_params* prm,
                              int64_t* sums) {
  svo_ctx* ctx = t.ctx;
  SvoProfScope prof(ctx, SVO_PROF_VOXEL_ALIGN);
  SVO_HIP_CHECK(ctx, hipMemsetAsync(sums, 0, VOXEL_ALIGN_WORDS * sizeof(int64_t), ctx->stream));
  if (n == 0) return SVO_OK;
  VoxelAlignArgs a{};
  a.pts = points; a.n = n;
  memcpy(a.m, c2w12, sizeof(a.m));
  a.voxel_size = t.voxel_size; a.max_depth = t.max_depth;
  a.keys = t.keys; a.ci = t.ci; a.sx = t.sx; a.sy = t.sy; a.sz = t.sz;
  a.mask = t.mask;
  a.min_count = (unsigned)prm->min_count;
  a.max_d2 = (double)prm->max_dist * (double)prm->max_dist;
  a.sums = reinterpret_cast<u64*>(sums);
  const dim3 grid((unsigned)voxel_align_groups(n)), block(VA_T);
  if (prm->reach == 0) hipLaunchKernelGGL(voxel_align_kernel<1>, grid, block, 0, ctx->stream, a);
  else hipLaunchKernelGGL(voxel_align_kernel<27>, grid, block, 0, ctx->stream, a);
  SVO_HIP_CHECK(ctx, hipGetLastError());
  return SVO_OK;
}

extern "C" int svo_voxel_map_align_sums_dev(svo_voxel_map* m, const svo_cloud_point* points, int n, const double* c2w12,
                                            const svo_voxel_align_params* prm, int64_t* sums) {
  if (!m) return SVO_ERR_INVALID;
  const SvoVoxelView t = svo_voxel_map_view(m);
  svo_use_device(t.ctx);
  SVO_ARGS_CHECK(t.ctx, voxel_align_sums_check(points, n, c2w12, prm, sums, &err));
  return voxel_align_launch(t, points, n, c2w12, prm, sums);
}

extern "C" int svo_voxel_map_align_sums_pose7_dev(svo_voxel_map* m, const svo_cloud_point* points, int n, const double* pose7,
                                                  const svo_voxel_align_params* prm, int64_t* sums) {
  if (!m) return SVO_ERR_INVALID;
  svo_ctx* ctx = svo_voxel_map_view(m).ctx;
  SVO_ARGS_CHECK(ctx, voxel_align_n_check(n, &err));
  SVO_REQUIRE(ctx, pose7, "voxel_map_align: null pose7");
  double m12[12];
  voxel_pose7_to_cam_to_world(pose7, m12);
  return svo_voxel_map_align_sums_dev(m, points, n, m12, prm, sums);
}

extern "C" int svo_voxel_map_align(svo_voxel_map* m, const svo_cloud_point* points, int n, const double* pose7_in,
                                   const svo_voxel_align_params* prm, double* pose7_out, svo_voxel_align_result* result) {
  if (!m) return SVO_ERR_INVALID;
  const SvoVoxelView t = svo_voxel_map_view(m);
  svo_ctx* ctx = t.ctx;
  svo_use_device(ctx);
  SVO_ARGS_CHECK(ctx, voxel_align_loop_check(points, n, pose7_in, prm, pose7_out, result, &err));
  SvoScratch scratch(ctx);
  int64_t* d = scratch.take<int64_t>(VOXEL_ALIGN_WORDS);  // the context's scratch: every iteration ends with the stream drained
  SVO_REQUIRE(ctx, d, "voxel_map_align: the context has no scratch");
  return voxel_align_loop(
      pose7_in, prm,
      [&](const double* m12, int64_t* w) {
        return svo_host_call(
            ctx, "voxel_map_align", hipSuccess, [&] { return voxel_align_launch(t, points, n, m12, prm, d); },
            [&] { return hipMemcpyAsync(w, d, VOXEL_ALIGN_WORDS * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream); });
      },
      pose7_out, result);
}
