// Ground plan view (include/svo.h, "Ground plan view"): from each of up to 4,096 candidate cells of a u8 class grid the
// cells inside max_range that a straight line reaches before an OPAQUE cell stops it, how many of them are GAIN, the score of that
// against the cost of getting there, the candidates ranked and the best one named, on the context's stream.  Two memsets and two
// launches:
//
//   view_cast_kernel : one workgroup of 1,024 per view.  An ignored view (rule 2) writes its record and leaves.  A used one stages the
//                      (2R + 1)^2 window of cls around it into LDS as two bit planes, OPAQUE and GAIN, a word of 32 cells per thread
//                      and turn; then every thread takes targets tid, tid + 1024, ... in ring order (host/view_args.h), so that the
//                      lanes of a wavefront walk lines of nearly equal length, and walks rule 3's line with integer remainders, the
//                      two bit look-ups per step in LDS, leaving at the first blocking cell.  A visible cell issues one atomicMin of
//                      the view's index on seen[cell]; the lane that found NONE there counts the cell as newly covered.  Tallies by
//                      __ballot / __popcll per wavefront, one LDS add per wavefront and tally, one record, one slot for the rank and
//                      one global add per non-zero count per workgroup.  STAGED false (svo_grid_view_set_mode, a measurement aid) is
//                      the same body with every look-up a read of cls.
//   view_rank_kernel : one workgroup.  key = score << 32 | (0xFFFFFFFF - i) per view into LDS; every view counts the keys larger than
//                      its own: its rank, a permutation because the keys are distinct; order[rank] = i, rank 0 writes best.
//
// How the workgroups of one launch agree (docs/HISTORY.md, "No cache maintenance inside kernels"): only through relaxed
// device-scope integer atomics whose final value does not depend on order (min, add).  No fence, no spinning, no persistent kernel;
// every loop is bounded by max_range <= 255 or n_views <= 4096 whatever memory holds; a view index is range-checked before anything
// is read through it, and every cell a line touches lies in the bounding box of the view and an in-grid target.
// Checks, sizes, the workspace's layout, the window's geometry, the ring enumeration and the score are host/view_args.h's.
#include "view_args.h"
#include "kernels.h"

namespace {
using u64 = unsigned long long;
constexpr int VW_T = VIEW_THREADS, VW_CT = VIEW_CAST_THREADS;
constexpr uint32_t VW_NONE = VIEW_NONE;
constexpr int VW_KEYS_PER_THREAD = VIEW_MAX_VIEWS / VW_T;

struct ViewSlot { uint32_t cell, n_gain, score, reserved; };  // what the cast leaves the rank per view
static_assert(sizeof(ViewSlot) == VIEW_SLOT_BYTES, "the workspace's layout of host/view_args.h");
static_assert(sizeof(svo_grid_view_rec) == 32, "the record of include/svo.h");
static_assert(VIEW_MAX_VIEWS % VW_T == 0, "the rank's keys per thread");

struct ViewArgs {
  const uint8_t* cls;
  const uint32_t* views;
  const uint32_t* cost;        // or null
  ViewSlot* slots;             // the workspace
  uint32_t* seen;              // the output or its stand-in in the workspace; null when neither seen nor counts is asked for
  svo_grid_view_rec* records;  // the outputs, null each
  uint32_t* order;
  uint32_t* best;
  u64* counts;                 // or null
  uint32_t n;                  // na * nb, at most 2^24
  int na, nb, n_views, range;
  uint32_t range2, opaque_mask, gain_mask, gain_weight, cost_div;
  uint32_t targets, rounds;
  int row_words, plane_words;
};

__device__ __forceinline__ bool vw_is(uint32_t mask, unsigned c) { return c < 32u && ((mask >> (c & 31u)) & 1u) != 0u; }

// One view's look-ups at the offset (da, db) from it, |da|, |db| <= range and the cell inside the grid.
template <bool STAGED>
struct ViewLook {
  const ViewArgs& a;
  const uint32_t* win;  // the two planes in LDS
  int va, vb;
  __device__ __forceinline__ unsigned cls_at(int da, int db) const { return a.cls[(size_t)(va + da) * (size_t)a.nb + (size_t)(vb + db)]; }
  __device__ __forceinline__ bool bit(int plane, int da, int db) const {
    const int la = a.range + da, lb = a.range + db;
    return ((win[plane * a.plane_words + la * a.row_words + (lb >> 5)] >> (lb & 31)) & 1u) != 0u;
  }
  __device__ __forceinline__ bool opaque(int da, int db) const { return STAGED ? bit(0, da, db) : vw_is(a.opaque_mask, cls_at(da, db)); }
  __device__ __forceinline__ bool gain(int da, int db) const { return STAGED ? bit(1, da, db) : vw_is(a.gain_mask, cls_at(da, db)); }
};

// Rule 4 for a target inside the grid and the range: rule 3's line by remainders, r = (2 i |d| + n) mod 2n and the quotient beside it.
template <bool STAGED>
__device__ __forceinline__ bool vw_visible(const ViewLook<STAGED>& look, int da, int db) {
  const int ada = da < 0 ? -da : da, adb = db < 0 ? -db : db, sa = da < 0 ? -1 : 1, sb = db < 0 ? -1 : 1;
  const int n = ada > adb ? ada : adb;
  int ra = n, rb = n, pa = 0, pb = 0;  // L_0 = V
  for (int i = 1; i <= n; ++i) {       // n <= 255
    int qa = pa, qb = pb;
    ra += 2 * ada; if (ra >= 2 * n) { ra -= 2 * n; ++qa; }
    rb += 2 * adb; if (rb >= 2 * n) { rb -= 2 * n; ++qb; }
    if (qa != pa && qb != pb && look.opaque(sa * qa, sb * pb) && look.opaque(sa * pa, sb * qb)) return false;  // a closed corner
    if (i < n && look.opaque(sa * qa, sb * qb)) return false;
    pa = qa; pb = qb;
  }
  return true;
}
}  // namespace

template <bool STAGED>
__global__ __launch_bounds__(VW_CT) void view_cast_kernel(ViewArgs a) {
  extern __shared__ uint32_t sWin[];  // STAGED: the OPAQUE plane, then the GAIN plane
  __shared__ unsigned sN[6];          // in range, visible, gain, opaque, newly covered, newly covered and gain
  constexpr int DEV = __HIP_MEMORY_SCOPE_AGENT;
  const int tid = threadIdx.x;
  const uint32_t i = blockIdx.x;
  const uint32_t v = a.views[i];
  bool used = v < a.n;                // before anything is read through it
  if (used) used = !vw_is(a.opaque_mask, a.cls[v]);
  if (!used) {                        // uniform over the workgroup
    if (tid == 0) {
      if (a.records) {
        svo_grid_view_rec r;
        r.cell = VW_NONE; r.n_visible = r.n_gain = r.n_opaque = 0u; r.cost = VW_NONE; r.score = 0u; r.reserved[0] = r.reserved[1] = 0u;
        a.records[i] = r;
      }
      a.slots[i] = ViewSlot{VW_NONE, 0u, 0u, 0u};
      if (a.counts) __hip_atomic_fetch_add(&a.counts[1], 1ull, __ATOMIC_RELAXED, DEV);
    }
    return;
  }
  const int va = (int)(v / (uint32_t)a.nb), vb = (int)(v - (uint32_t)va * (uint32_t)a.nb);
  if (tid < 6) sN[tid] = 0u;
  if (STAGED) {
    const int side = 2 * a.range + 1;
    for (int idx = tid; idx < a.plane_words; idx += VW_CT) {
      const int row = idx / a.row_words, w = idx - row * a.row_words;
      const int ga = va - a.range + row;
      uint32_t o = 0u, g = 0u;
      if (ga >= 0 && ga < a.na) {
        const int lb0 = 32 * w, gb0 = vb - a.range + lb0;
        const uint8_t* const line = a.cls + (size_t)ga * (size_t)a.nb;
        for (int bit = 0; bit < 32; ++bit) {
          const int gb = gb0 + bit;
          if (gb < 0 || gb >= a.nb || lb0 + bit >= side) continue;  // outside the grid a bit reads as "not there"
          const unsigned c = line[gb];
          o |= vw_is(a.opaque_mask, c) ? 1u << bit : 0u;
          g |= vw_is(a.gain_mask, c) ? 1u << bit : 0u;
        }
      }
      sWin[idx] = o;
      sWin[a.plane_words + idx] = g;
    }
  }
  __syncthreads();
  const ViewLook<STAGED> look{a, sWin, va, vb};
  unsigned n_in = 0, n_vis = 0, n_gain = 0, n_opq = 0, n_cov = 0, n_gcov = 0;  // the same in every lane of a wavefront
  for (uint32_t round = 0; round < a.rounds; ++round) {  // the same trip count for every thread
    const uint32_t t = round * VW_CT + (uint32_t)tid;
    int da = 0, db = 0;
    if (t < a.targets) view_target_cell(t, &da, &db);
    const int ta = va + da, tb = vb + db;
    const bool in = t < a.targets && ta >= 0 && ta < a.na && tb >= 0 && tb < a.nb && (uint32_t)(da * da + db * db) <= a.range2;
    const bool vis = in && vw_visible<STAGED>(look, da, db);
    const bool gain = vis && look.gain(da, db), opq = vis && look.opaque(da, db);
    bool fresh = false;
    if (vis && a.seen) fresh = __hip_atomic_fetch_min(&a.seen[(size_t)ta * (size_t)a.nb + (size_t)tb], i, __ATOMIC_RELAXED, DEV) == VW_NONE;
    n_in += (unsigned)__popcll(__ballot(in));
    n_vis += (unsigned)__popcll(__ballot(vis));
    n_gain += (unsigned)__popcll(__ballot(gain));
    n_opq += (unsigned)__popcll(__ballot(opq));
    n_cov += (unsigned)__popcll(__ballot(fresh));
    n_gcov += (unsigned)__popcll(__ballot(fresh && gain));
  }
  if ((tid & 63) == 0) {
    constexpr int WG = __HIP_MEMORY_SCOPE_WORKGROUP;
    __hip_atomic_fetch_add(&sN[0], n_in, __ATOMIC_RELAXED, WG);
    __hip_atomic_fetch_add(&sN[1], n_vis, __ATOMIC_RELAXED, WG);
    __hip_atomic_fetch_add(&sN[2], n_gain, __ATOMIC_RELAXED, WG);
    __hip_atomic_fetch_add(&sN[3], n_opq, __ATOMIC_RELAXED, WG);
    __hip_atomic_fetch_add(&sN[4], n_cov, __ATOMIC_RELAXED, WG);
    __hip_atomic_fetch_add(&sN[5], n_gcov, __ATOMIC_RELAXED, WG);
  }
  __syncthreads();
  if (tid == 0) {
    const uint32_t c = a.cost ? a.cost[v] : VW_NONE;
    const uint32_t score = view_score(sN[2], c, a.cost != nullptr, a.gain_weight, a.cost_div);
    if (a.records) {
      svo_grid_view_rec r;
      r.cell = v; r.n_visible = sN[1]; r.n_gain = sN[2]; r.n_opaque = sN[3]; r.cost = c; r.score = score; r.reserved[0] = r.reserved[1] = 0u;
      a.records[i] = r;
    }
    a.slots[i] = ViewSlot{v, sN[2], score, 0u};
  }
  if (a.counts && tid < 6) {  // n_used, then n_in_range, n_visible, n_gain, n_covered, n_gain_covered: counts[0], [2] .. [6]
    const unsigned t = tid == 0 ? 1u : sN[tid <= 3 ? tid - 1 : tid];  // the opaque tally, sN[3], is the record's alone
    if (t) __hip_atomic_fetch_add(&a.counts[tid == 0 ? 0 : tid + 1], (u64)t, __ATOMIC_RELAXED, DEV);
  }
}

__global__ __launch_bounds__(VW_T) void view_rank_kernel(ViewArgs a) {
  __shared__ u64 sKey[VIEW_MAX_VIEWS];
  const int tid = threadIdx.x;
  for (int j = tid; j < a.n_views; j += VW_T) sKey[j] = (u64)a.slots[j].score << 32 | (u64)(VW_NONE - (uint32_t)j);
  __syncthreads();
  u64 mine[VW_KEYS_PER_THREAD];
  uint32_t rank[VW_KEYS_PER_THREAD];
#pragma unroll
  for (int q = 0; q < VW_KEYS_PER_THREAD; ++q) {
    const int j = tid + q * VW_T;
    mine[q] = j < a.n_views ? sKey[j] : ~0ull;
    rank[q] = 0u;
  }
  for (int j = 0; j < a.n_views; ++j) {  // n_views <= 4096; every lane reads the same word
    const u64 k = sKey[j];
#pragma unroll
    for (int q = 0; q < VW_KEYS_PER_THREAD; ++q) rank[q] += k > mine[q] ? 1u : 0u;
  }
#pragma unroll
  for (int q = 0; q < VW_KEYS_PER_THREAD; ++q) {
    const int j = tid + q * VW_T;
    if (j >= a.n_views) continue;
    // the keys are distinct in their low words, so rank[q] < n_views whatever the slots hold
    if (a.order) a.order[rank[q]] = (uint32_t)j;
    if (rank[q] == 0u && a.best) {
      const ViewSlot s = a.slots[j];
      const bool some = s.score > 0u;
      a.best[0] = some ? s.cell : VW_NONE;
      a.best[1] = some ? (uint32_t)j : VW_NONE;
      a.best[2] = some ? s.score : 0u;
      a.best[3] = some ? s.n_gain : 0u;
    }
  }
}

// ----------------------------------------------------------------------------- host side
extern "C" int svo_grid_view_default_params(const svo_grid_clearance_params* clearance, svo_grid_view_params* out) {
  return view_default_params(clearance, out);
}

extern "C" size_t svo_grid_view_workspace_bytes(int na, int nb, int n_views) { return view_workspace_bytes(na, nb, n_views); }

extern "C" int svo_grid_view_set_mode(svo_ctx* ctx, int staged) {
  if (!ctx) return SVO_ERR_INVALID;
  ctx->view_staged = staged ? 1 : 0;
  return SVO_OK;
}

extern "C" int svo_grid_view_dev(svo_ctx* ctx, const uint8_t* cls, const uint32_t* views, int n_views, const uint32_t* cost,
                                 const svo_grid_view_params* prm, void* workspace, const svo_grid_view_out* out, uint64_t* counts) {
  if (!ctx) return SVO_ERR_INVALID;
  svo_use_device(ctx);
  SVO_ARGS_CHECK(ctx, view_check(cls, views, n_views, cost, prm, workspace, out, counts, true, &err));
  const int na = prm->na, nb = prm->nb, range = prm->max_range;
  unsigned char* const ws = static_cast<unsigned char*>(workspace);
  ViewArgs a{};
  a.cls = cls; a.views = views; a.cost = cost;
  a.slots = reinterpret_cast<ViewSlot*>(ws + view_ws_slots_offset());
  // the cover counts need the array whether or not it is asked for
  a.seen = out->seen ? out->seen : counts ? reinterpret_cast<uint32_t*>(ws + view_ws_seen_offset(n_views)) : nullptr;
  a.records = out->records; a.order = out->order; a.best = out->best;
  a.counts = reinterpret_cast<u64*>(counts);
  a.n = (uint32_t)na * (uint32_t)nb; a.na = na; a.nb = nb; a.n_views = n_views; a.range = range;
  a.range2 = (uint32_t)(range * range); a.opaque_mask = prm->opaque_mask; a.gain_mask = prm->gain_mask;
  a.gain_weight = prm->gain_weight; a.cost_div = prm->cost_div;
  a.targets = view_targets(range); a.rounds = view_target_rounds(range);
  a.row_words = view_window_row_words(range); a.plane_words = view_window_plane_words(range);
  const bool staged = ctx->view_staged != 0;
  const size_t lds = staged ? view_lds_bytes(range) : 0;
  static_assert(2 * sizeof(uint32_t) * (2 * VIEW_MAX_RANGE + 1) * ((2 * VIEW_MAX_RANGE + 1 + 31) / 32) + 64 <= VIEW_LDS_LIMIT, "the window fits");
  const dim3 wg(VW_T), cast_wg(VW_CT);
  hipStream_t st = ctx->stream;
  SvoProfScope prof(ctx, SVO_PROF_GRID_VIEW);
  if (counts) SVO_HIP_CHECK(ctx, hipMemsetAsync(counts, 0, 8 * sizeof(u64), st));
  if (a.seen) SVO_HIP_CHECK(ctx, hipMemsetAsync(a.seen, 0xFF, sizeof(uint32_t) * (size_t)na * (size_t)nb, st));
  if (staged) hipLaunchKernelGGL(view_cast_kernel<true>, dim3((unsigned)n_views), cast_wg, lds, st, a);
  else hipLaunchKernelGGL(view_cast_kernel<false>, dim3((unsigned)n_views), cast_wg, 0, st, a);
  if (a.order || a.best) hipLaunchKernelGGL(view_rank_kernel, dim3(1), wg, 0, st, a);
  SVO_HIP_CHECK(ctx, hipGetLastError());
  return SVO_OK;
}

extern "C" int svo_grid_view(svo_ctx* ctx, const uint8_t* cls, const uint32_t* views, int n_views, const uint32_t* cost,
                             const svo_grid_view_params* prm, const svo_grid_view_out* out, uint64_t* counts) {
  if (!ctx) return SVO_ERR_INVALID;
  svo_use_device(ctx);
  SVO_ARGS_CHECK(ctx, view_check(cls, views, n_views, cost, prm, nullptr, out, counts, false, &err));
  const size_t n = (size_t)prm->na * (size_t)prm->nb, nv = (size_t)n_views, b_rec = nv * sizeof(svo_grid_view_rec);
  SvoParts parts;
  const size_t o_counts = parts.add(8 * sizeof(u64)), o_ws = parts.add(view_workspace_bytes(prm->na, prm->nb, n_views)), o_rec = parts.add(b_rec),
               o_order = parts.add(4 * nv), o_best = parts.add(16), o_seen = parts.add(4 * n), o_views = parts.add(4 * nv), o_cost = parts.add(4 * n),
               o_cls = parts.add(n);
  SvoTemp d;
  SVO_HIP_CHECK(ctx, hipMalloc(&d.p, parts.total()));
  svo_grid_view_out o{};
  o.records = out->records ? d.at<svo_grid_view_rec>(o_rec) : nullptr;  // what the caller did not ask for is not written
  o.order = out->order ? d.at<uint32_t>(o_order) : nullptr;
  o.best = out->best ? d.at<uint32_t>(o_best) : nullptr;
  o.seen = out->seen ? d.at<uint32_t>(o_seen) : nullptr;
  u64 c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  hipStream_t st = ctx->stream;
  hipError_t e = hipMemcpyAsync(d.at(o_cls), cls, n, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d.at(o_views), views, 4 * nv, hipMemcpyHostToDevice, st);
  if (e == hipSuccess && cost) e = hipMemcpyAsync(d.at(o_cost), cost, 4 * n, hipMemcpyHostToDevice, st);
  const int rc = svo_host_call(
      ctx, "grid_view", e,
      [&] {
        return svo_grid_view_dev(ctx, d.at(o_cls), d.at<uint32_t>(o_views), n_views, cost ? d.at<uint32_t>(o_cost) : nullptr, prm, d.at(o_ws), &o,
                                 counts ? d.at<uint64_t>(o_counts) : nullptr);
      },
      [&] {
        hipError_t e = hipSuccess;
        if (out->records) e = hipMemcpyAsync(out->records, o.records, b_rec, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && out->order) e = hipMemcpyAsync(out->order, o.order, 4 * nv, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && out->best) e = hipMemcpyAsync(out->best, o.best, 16, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && out->seen) e = hipMemcpyAsync(out->seen, o.seen, 4 * n, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && counts) e = hipMemcpyAsync(c, d.at(o_counts), sizeof(c), hipMemcpyDeviceToHost, st);
        return e;
      });
  if (rc) return rc;
  if (counts) for (int k = 0; k < 8; ++k) counts[k] = c[k];
  return SVO_OK;
}
