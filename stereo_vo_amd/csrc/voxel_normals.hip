// Voxel map normals (include/svo.h, "Voxel map normals"): every voxel gets a normal and a curvature from the means of
// the 27 voxels around it, into a side array of the caller's with one 16-byte record per slot.
//
//   voxel_normals_kernel : 256-thread workgroups; a workgroup owns a contiguous run of VOXEL_NORMALS_RUN slots per thread.  The heavy
//                          work is 26 look-ups and a Jacobi per LIVE slot, and a table at a sensible load is half empty or more, so the
//                          lanes do not walk the slots one each:
//                            1  the run's keys and count | intensity words are loaded coalesced; a slot that is no centre gets its
//                               {0, 0, 0, -1} record at once; the centres' slot numbers and keys are compacted into LDS (ballot and
//                               prefix per wavefront, the wavefronts' totals through one LDS word per pass and wavefront and ONE barrier);
//                            2  the threads take centres densely from that list.  The look-up is csrc/voxel_align.hip's, phase by
//                               phase (A the 27 home slots' keys in one run of loads, B found / foreign as two bit masks, C the counts
//                               and D the sums with the ADDRESS selected, nine candidates at a time, E the rare probe continuation as a
//                               loop over the foreign mask), with two differences: a candidate whose index leaves the key range is
//                               absent (it reads the centre's slot and is dropped), and the centre candidate is the slot itself,
//                               wherever in its probe run it sits.  The participants' integer moments, the Jacobi, the validity tests
//                               and the record are host/voxel_normals.h, the text a CPU program runs too.
//                          No array is indexed by a run-time value (scratch 0).  The five counts are summed per thread, then through a
//                          __shfl_xor tree per wavefront, one LDS row per wavefront, and one relaxed atomicAdd per workgroup and
//                          non-zero word.
//
// §7c's conditions: relaxed device-scope atomics only (the counts), no fence, no waiting on another workgroup, scratch 0.  The launch
// claims nothing and writes nothing but the caller's records and counts: every key it reads was written by an earlier launch on the
// same stream, so a load decides (csrc/voxel.hip, vx_find).  csrc/voxel_align.hip is untouched: its few-line helpers (hash, offset
// load) are restated here rather than moved, so its two instantiations compile to what they did.
#include "kernels.h"
#include "voxel_normals.h"

namespace {
typedef unsigned long long u64;
typedef long long i64;
constexpr int VN_T = VOXEL_THREADS;
constexpr int VN_RUN = VOXEL_NORMALS_RUN;
constexpr int VN_SLOTS = VN_T * VN_RUN;  // slots per workgroup
constexpr int VN_WAVES = VN_T / 64;
constexpr u64 VN_EMPTY = ~0ull;
constexpr int VN_NC = 27, VN_CENTRE = 13, VN_G = 9;

struct VoxelNormalsArgs {
  const u64 *keys, *ci, *sx, *sy, *sz;
  u64 mask;  // cap - 1
  unsigned min_count;
  int min_neighbours;
  float max_curvature;
  svo_voxel_normal* normals;
  u64* counts;  // 8 words, zeroed on the stream before the launch; or null
};

__device__ __forceinline__ u64 vn_fmix64(u64 k) {  // the voxel map's hash (include/svo.h, "voxel map": Table)
  k ^= k >> 33; k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return k;
}

// The word at byte offset `off` of one of the table's arrays: a slot index is below 2^28, so its byte offset fits 32 bits.
__device__ __forceinline__ u64 vn_at(const u64* base, unsigned off) { return *reinterpret_cast<const u64*>(reinterpret_cast<const char*>(base) + off); }
__device__ __forceinline__ unsigned vn_hi(const u64* base, unsigned off) { return *reinterpret_cast<const unsigned*>(reinterpret_cast<const char*>(base) + off + 4u); }

// Candidate c: the key of k + (c % 3 - 1, c / 3 % 3 - 1, c / 9 - 1).  Only meaningful where vn_in_range says so.
__device__ __forceinline__ u64 vn_key(u64 base, int c) {
  const i64 i = c % 3 - 1, j = c / 3 % 3 - 1, l = c / 9 - 1;
  return (u64)((i64)base + i + j * (1ll << 21) + l * (1ll << 42));
}

// Bit c set iff no index of candidate c leaves [-2^20, 2^20), i.e. no 21-bit field of the key under- or overflows.
__device__ __forceinline__ unsigned vn_in_range(u64 base) {
  unsigned m = (1u << VN_NC) - 1u;
  const unsigned f0 = (unsigned)(base & 0x1FFFFFull), f1 = (unsigned)((base >> 21) & 0x1FFFFFull), f2 = (unsigned)((base >> 42) & 0x1FFFFFull);
  constexpr unsigned I_LO = 0x1249249u, I_HI = I_LO << 2;                 // candidates with i = -1 / i = +1
  constexpr unsigned J_LO = 0x7u | 0x7u << 9 | 0x7u << 18, J_HI = J_LO << 6;  // j = -1 / j = +1
  constexpr unsigned L_LO = 0x1FFu, L_HI = 0x1FFu << 18;                  // l = -1 / l = +1
  if (f0 == 0u) m &= ~I_LO;
  if (f0 == 0x1FFFFFu) m &= ~I_HI;
  if (f1 == 0u) m &= ~J_LO;
  if (f1 == 0x1FFFFFu) m &= ~J_HI;
  if (f2 == 0u) m &= ~L_LO;
  if (f2 == 0x1FFFFFu) m &= ~L_HI;
  return m;
}

__global__ __launch_bounds__(VN_T) void voxel_normals_kernel(VoxelNormalsArgs a) {
  __shared__ unsigned sCnt[VN_RUN][VN_WAVES];
  __shared__ unsigned sSlot[VN_SLOTS];
  __shared__ u64 sKey[VN_SLOTS];
  __shared__ unsigned sW[VN_WAVES][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const u64 cap = a.mask + 1ull;
  const u64 first = (u64)blockIdx.x * (u64)VN_SLOTS;
  const float4 none = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
  // 1: the run's slots, coalesced; the records of the slots that are no centres; the centres compacted
  u64 key[VN_RUN];
  unsigned before[VN_RUN];  // centres in the lanes below this one, per pass
  bool centre[VN_RUN];
#pragma unroll
  for (int it = 0; it < VN_RUN; ++it) {
    const u64 slot = first + (u64)(it * VN_T + tid);
    const bool in = slot < cap;
    key[it] = in ? a.keys[slot] : VN_EMPTY;
    const u64 ci = in ? a.ci[slot] : 0ull;
    centre[it] = key[it] != VN_EMPTY && (ci >> 40) >= (u64)a.min_count;
    if (in && !centre[it]) reinterpret_cast<float4*>(a.normals)[slot] = none;
    const u64 b = __ballot(centre[it]);
    before[it] = (unsigned)__popcll(b & ((1ull << lane) - 1ull));
    if (lane == 0) sCnt[it][wave] = (unsigned)__popcll(b);
  }
  __syncthreads();
  unsigned total = 0;
#pragma unroll
  for (int it = 0; it < VN_RUN; ++it) {
    unsigned at = 0;
#pragma unroll
    for (int wv = 0; wv < VN_WAVES; ++wv) {  // the (pass, wavefront) pairs in list order: one running sum
      at = wv == wave ? total : at;
      total += sCnt[it][wv];
    }
    if (centre[it]) {
      sSlot[at + before[it]] = (unsigned)(it * VN_T + tid);  // relative to `first`: below VN_SLOTS
      sKey[at + before[it]] = key[it];
    }
  }
  __syncthreads();
  // 2: the centres, densely
  unsigned verdicts[4] = {0u, 0u, 0u, 0u};  // valid, few, collinear, curved of this thread's centres
  for (unsigned idx = (unsigned)tid; idx < total; idx += (unsigned)VN_T) {
    const u64 slot = first + (u64)sSlot[idx];
    const u64 base = sKey[idx];
    const unsigned own = (unsigned)slot << 3;  // the centre's own byte offset: what an absent candidate reads instead
    const unsigned inr = vn_in_range(base);
    // A: every home slot's key, asked for before any is waited for
    unsigned h[VN_NC];
    u64 got[VN_NC];
#pragma unroll
    for (int c = 0; c < VN_NC; ++c) {
      const unsigned home = (unsigned)(vn_fmix64(vn_key(base, c)) & a.mask) << 3;
      h[c] = c == VN_CENTRE || !(inr >> c & 1u) ? own : home;
    }
#pragma unroll
    for (int c = 0; c < VN_NC; ++c) got[c] = vn_at(a.keys, h[c]);
    // B: found at home / foreign at home (the keys are formed again from a copy of base the compiler cannot see through, as in
    // csrc/voxel_align.hip: kept from phase A they hold 54 registers to the end)
    unsigned found = 0, foreign = 0;
    u64 base_b = base;
    asm volatile("" : "+v"(base_b));
#pragma unroll
    for (int c = 0; c < VN_NC; ++c) {
      const u64 k = vn_key(base_b, c);
      const bool there = (inr >> c & 1u) != 0u;
      found |= there && got[c] == k ? 1u << c : 0u;
      foreign |= there && got[c] != k && got[c] != VN_EMPTY ? 1u << c : 0u;
    }
    // C: the counts of the slots found at home, all in flight: the address is selected, not the load
    unsigned count[VN_NC];
#pragma unroll
    for (int c = 0; c < VN_NC; ++c) count[c] = vn_hi(a.ci, found >> c & 1u ? h[c] : own);
#pragma unroll
    for (int c = 0; c < VN_NC; ++c) count[c] = found >> c & 1u ? count[c] >> 8 : 0u;  // the count is bits 40..63; carved: 0
    // D: the sums of the participants by the same selection, nine candidates at a time (the centre's count is >= min_count)
    VoxelMoments mo;
    voxel_moments_clear(mo);
#pragma unroll
    for (int g0 = 0; g0 < VN_NC; g0 += VN_G) {
      u64 s[VN_G][3];
#pragma unroll
      for (int c = 0; c < VN_G; ++c) {
        const unsigned at = count[g0 + c] >= a.min_count ? h[g0 + c] : own;
        s[c][0] = vn_at(a.sx, at); s[c][1] = vn_at(a.sy, at); s[c][2] = vn_at(a.sz, at);
      }
#pragma unroll
      for (int c = 0; c < VN_G; ++c) {
        const int cc = g0 + c;
        if (count[cc] >= a.min_count) voxel_moments_add(mo, cc % 3 - 1, cc / 3 % 3 - 1, cc / 9 - 1, count[cc], s[c][0], s[c][1], s[c][2]);
      }
    }
    // E: the rare continuation: candidates whose home slot holds another key
    while (foreign) {
      const int c = __builtin_ctz(foreign);
      foreign &= foreign - 1u;
      const u64 k = vn_key(base, c);
      u64 at = vn_fmix64(k) & a.mask;
      for (int p = 1; p < SVO_VOXEL_MAX_PROBES; ++p) {  // the home slot was probe 0
        at = (at + 1ull) & a.mask;
        const u64 kk = a.keys[at];
        if (kk == VN_EMPTY) break;
        if (kk == k) {
          const u64 cnt = a.ci[at] >> 40;
          if (cnt >= (u64)a.min_count) voxel_moments_add(mo, c % 3 - 1, c / 3 % 3 - 1, c / 9 - 1, (unsigned)cnt, a.sx[at], a.sy[at], a.sz[at]);
          break;
        }
      }
    }
    svo_voxel_normal rec;
    const int verdict = voxel_normal_finish(mo, a.min_neighbours, a.max_curvature, &rec);
    reinterpret_cast<float4*>(a.normals)[slot] = make_float4(rec.nx, rec.ny, rec.nz, rec.curvature);
    verdicts[0] += verdict == VOXEL_NORMAL_VALID ? 1u : 0u;
    verdicts[1] += verdict == VOXEL_NORMAL_FEW ? 1u : 0u;
    verdicts[2] += verdict == VOXEL_NORMAL_COLLINEAR ? 1u : 0u;
    verdicts[3] += verdict == VOXEL_NORMAL_CURVED ? 1u : 0u;
  }
  // the counts: wavefront tree, one LDS row per wavefront, one atomicAdd per workgroup and non-zero word
  if (!a.counts) return;  // uniform
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int k = 0; k < 4; ++k) verdicts[k] += __shfl_xor(verdicts[k], o);
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) sW[wave][k] = verdicts[k];
  }
  __syncthreads();
  if (tid < 5) {  // word 0 is n_centres; word t > 0 is verdict t - 1
    u64 t = tid == 0 ? (u64)total : 0ull;
    if (tid > 0) {
      for (int wv = 0; wv < VN_WAVES; ++wv) t += sW[wv][tid - 1];
    }
    if (t) __hip_atomic_fetch_add(&a.counts[tid], t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}
}  // namespace

// ----------------------------------------------------------------------------- host side
extern "C" int svo_voxel_normals_default_params(svo_voxel_normals_params* params) { return voxel_normals_default_params(params); }
extern "C" int svo_voxel_map_normals_bytes(const svo_voxel_map_params* params, size_t* bytes) { return voxel_normals_bytes(params, bytes); }

// The memset and the launch of checked arguments.
static int voxel_normals_launch(const SvoVoxelView& t, const svo_voxel_normals_params* prm, svo_voxel_normal* normals, uint64_t* counts) {
  svo_ctx* ctx = t.ctx;
  SvoProfScope prof(ctx, SVO_PROF_VOXEL_NORMALS);
  if (counts) SVO_HIP_CHECK(ctx, hipMemsetAsync(counts, 0, VOXEL_NORMALS_COUNTS * sizeof(uint64_t), ctx->stream));
  VoxelNormalsArgs a{};
  a.keys = t.keys; a.ci = t.ci; a.sx = t.sx; a.sy = t.sy; a.sz = t.sz;
  a.mask = t.mask;
  a.min_count = (unsigned)prm->min_count;
  a.min_neighbours = prm->min_neighbours;
  a.max_curvature = prm->max_curvature;
  a.normals = normals;
  a.counts = reinterpret_cast<u64*>(counts);
  const dim3 grid((unsigned)voxel_normals_groups((size_t)t.mask + 1)), block(VN_T);
  hipLaunchKernelGGL(voxel_normals_kernel, grid, block, 0, ctx->stream, a);
  SVO_HIP_CHECK(ctx, hipGetLastError());
  return SVO_OK;
}

extern "C" int svo_voxel_map_normals_dev(svo_voxel_map* m, const svo_voxel_normals_params* prm, svo_voxel_normal* normals, uint64_t* counts) {
  if (!m) return SVO_ERR_INVALID;
  const SvoVoxelView t = svo_voxel_map_view(m);
  svo_use_device(t.ctx);
  SVO_ARGS_CHECK(t.ctx, voxel_normals_check(prm, normals, counts, true, &err));
  return voxel_normals_launch(t, prm, normals, counts);
}

extern "C" int svo_voxel_map_normals(svo_voxel_map* m, const svo_voxel_normals_params* prm, svo_voxel_normal* host_normals, uint64_t* host_counts) {
  if (!m) return SVO_ERR_INVALID;
  const SvoVoxelView t = svo_voxel_map_view(m);
  svo_ctx* ctx = t.ctx;
  svo_use_device(ctx);
  SVO_ARGS_CHECK(ctx, voxel_normals_check(prm, host_normals, host_counts, false, &err));
  const size_t bytes = VOXEL_NORMAL_BYTES * ((size_t)t.mask + 1);
  SvoParts parts;
  const size_t o_normals = parts.add(bytes), o_counts = parts.add(VOXEL_NORMALS_COUNTS * sizeof(uint64_t));
  SvoTemp d;
  SVO_HIP_CHECK(ctx, hipMalloc(&d.p, parts.total()));
  uint64_t c[VOXEL_NORMALS_COUNTS] = {};
  const int rc = svo_host_call(
      ctx, "voxel_map_normals", hipSuccess, [&] { return voxel_normals_launch(t, prm, d.at<svo_voxel_normal>(o_normals), d.at<uint64_t>(o_counts)); },
      [&] {
        hipError_t e = hipMemcpyAsync(host_normals, d.at(o_normals), bytes, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess && host_counts) e = hipMemcpyAsync(c, d.at(o_counts), sizeof(c), hipMemcpyDeviceToHost, ctx->stream);
        return e;
      });
  if (rc) return rc;
  if (host_counts) memcpy(host_counts, c, sizeof(c));
  return SVO_OK;
}
