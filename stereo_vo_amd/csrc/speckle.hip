// Speckle filter of CV_16S disparity maps (include/svo.h, "speckle filter"): every 4-connected component of
// similar disparity with at most max_size pixels becomes FILTERED (-16).  Connected-component labelling by union-find over a
// batch of maps, the pair index in the grid, four launches on the context's stream:
//
//   speckle_tile_kernel   : one workgroup labels one 64 x 16 tile with union-find in LDS (LDS atomicMin) and writes, per pixel,
//                           label = image index of its tile-local root (NONE for a FILTERED pixel) and count = the size of the
//                           tile-local component at its root, 0 everywhere else.
//   speckle_seam_kernel   : one thread per pair of 4-neighbours across a tile seam that satisfies the join rule: find both
//                           roots, then hook the larger under the smaller with atomicMin until the hook lands on a root.
//   speckle_count_kernel  : every tile-local root (count != 0) that is no longer a root adds its count to its root's.
//   speckle_apply_kernel  : a pixel whose root's count is <= max_size is written as FILTERED and counted.
//
// How the workgroups of one launch agree (docs/HISTORY.md, "No cache maintenance inside kernels"): only through relaxed
// device-scope integer atomics whose final value does not depend on order (atomicMin on labels, atomicAdd on counts).  No fence,
// no acquire / release, no loop whose exit depends on another workgroup's progress.  A plain load of a label may be stale: a
// label only ever decreases and every value it ever held is a pixel of the same component, so a stale value is a valid, merely
// longer, way to the root.  What a launch must see of another launch's plain stores comes from the kernel boundary.
#include "dense_args.h"
#include "kernels.h"

namespace {
constexpr int SP_FILTERED = -16;
constexpr unsigned SP_NONE = 0xFFFFFFFFu;
static_assert(SP_TW == 64 && SP_PIX % SP_T == 0, "a tile row is one wavefront; whole passes of the workgroup over the tile");

struct SpeckleArgs {
  int16_t* disp;    // batch tight maps, filtered in place by the apply pass
  unsigned* label;  // batch x A
  unsigned* count;  // batch x A
  int* n_removed;   // batch, or null
  int W, H, tiles_x, max_size, max_diff;
  unsigned n_vert, n_seam;  // seam pairs across vertical seams; all seam pairs
};

__device__ __forceinline__ bool joined(int a, int b, int max_diff) {
  return a != SP_FILTERED && b != SP_FILTERED && abs(a - b) <= max_diff;  // int32: |a - b| <= 65,535
}

__device__ __forceinline__ unsigned uf_find(const unsigned* L, unsigned x) {
  for (unsigned p; (p = L[x]) != x;) x = p;
  return x;
}

// Join the trees of a and b.  Each turn hooks the larger of two nodes under the smaller; when the larger was no root (old != a)
// its former parent `old` has to be joined with b instead, and max(a, b) has strictly decreased: at most a turns, no waiting.
template <int SCOPE>
__device__ __forceinline__ void uf_unite(unsigned* L, unsigned a, unsigned b) {
  a = uf_find(L, a);
  b = uf_find(L, b);
  while (a != b) {
    if (a < b) { const unsigned t = a; a = b; b = t; }
    const unsigned old = __hip_atomic_fetch_min(&L[a], b, __ATOMIC_RELAXED, SCOPE);
    if (old == a) break;
    a = old;
  }
}
}  // namespace

__global__ __launch_bounds__(SP_T) void speckle_tile_kernel(SpeckleArgs a) {
  __shared__ short sV[SP_PIX];
  __shared__ unsigned sL[SP_PIX], sC[SP_PIX];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int x0 = ((int)blockIdx.x % a.tiles_x) * SP_TW, y0 = ((int)blockIdx.x / a.tiles_x) * SP_TH;
  const size_t base = (size_t)b * (size_t)a.W * (size_t)a.H;
  const int16_t* disp = a.disp + base;
#pragma unroll
  for (int k = 0; k < SP_PIX / SP_T; ++k) {
    const int i = tid + k * SP_T, x = x0 + (i & (SP_TW - 1)), y = y0 + i / SP_TW;
    const int v = (x < a.W && y < a.H) ? (int)disp[(size_t)y * a.W + x] : SP_FILTERED;  // outside the image: no node
    sV[i] = (short)v;
    sL[i] = v != SP_FILTERED ? (unsigned)i : SP_NONE;
    sC[i] = 0;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < SP_PIX / SP_T; ++k) {
    const int i = tid + k * SP_T;
    const int v = sV[i];
    if ((i & (SP_TW - 1)) && joined(v, sV[i - 1], a.max_diff)) uf_unite<__HIP_MEMORY_SCOPE_WORKGROUP>(sL, i, i - 1);
    if (i >= SP_TW && joined(v, sV[i - SP_TW], a.max_diff)) uf_unite<__HIP_MEMORY_SCOPE_WORKGROUP>(sL, i, i - SP_TW);
  }
  __syncthreads();
  unsigned root[SP_PIX / SP_T];
#pragma unroll
  for (int k = 0; k < SP_PIX / SP_T; ++k) {
    const int i = tid + k * SP_T;
    root[k] = SP_NONE;
    if (sL[i] != SP_NONE) {
      root[k] = uf_find(sL, i);
      __hip_atomic_fetch_add(&sC[root[k]], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < SP_PIX / SP_T; ++k) {
    const int i = tid + k * SP_T, x = x0 + (i & (SP_TW - 1)), y = y0 + i / SP_TW;
    if (x >= a.W || y >= a.H) continue;
    const size_t p = base + (size_t)y * a.W + x;
    const unsigned r = root[k];
    a.label[p] = r == SP_NONE ? SP_NONE : (unsigned)((y0 + (int)(r / SP_TW)) * a.W + x0 + (int)(r & (SP_TW - 1)));
    a.count[p] = r == (unsigned)i ? sC[i] : 0u;
  }
  if (a.n_removed && blockIdx.x == 0 && tid == 0) a.n_removed[b] = 0;  // the apply pass adds to it two kernel boundaries later
}

// Seam pair j of an image: first the pairs (x - 1, x) across the vertical seams x = 64, 128, ..., then the pairs (y - 1, y) across
// the horizontal seams y = 16, 32, ...  A pair whose predecessor ALONG the seam is joined too and carries the same two labels is
// skipped: equal labels mean p ~ p' and q ~ q' already, and the predecessor's thread joins p' ~ q' (the first pair of such a run
// has no such predecessor, so it is never skipped).  On a long seam between two constant regions that leaves one hook, not 64.
__global__ __launch_bounds__(SP_T) void speckle_seam_kernel(SpeckleArgs a) {
  const unsigned j = blockIdx.x * SP_T + threadIdx.x;
  if (j >= a.n_seam) return;
  const size_t base = (size_t)blockIdx.y * (size_t)a.W * (size_t)a.H;
  const int16_t* disp = a.disp + base;
  unsigned* L = a.label + base;
  unsigned p, q, along;
  bool first;
  if (j < a.n_vert) {
    const unsigned s = j / (unsigned)a.H, y = j - s * (unsigned)a.H;
    q = y * (unsigned)a.W + (s + 1) * SP_TW; p = q - 1; along = (unsigned)a.W; first = y == 0;
  } else {
    const unsigned k = j - a.n_vert, s = k / (unsigned)a.W, x = k - s * (unsigned)a.W;
    q = (s + 1) * SP_TH * (unsigned)a.W + x; p = q - (unsigned)a.W; along = 1; first = x == 0;
  }
  if (!joined(disp[p], disp[q], a.max_diff)) return;
  // which pixels are nodes is the labelling pass's decision: a caller who breaks the contract and rewrites the map while the call
  // runs gets a meaningless result, never an index formed from NONE
  const unsigned lp = L[p], lq = L[q];
  if (lp == SP_NONE || lq == SP_NONE) return;
  if (!first && joined(disp[p - along], disp[q - along], a.max_diff) && L[p - along] == lp && L[q - along] == lq) return;
  uf_unite<__HIP_MEMORY_SCOPE_AGENT>(L, lp, lq);
}

__global__ __launch_bounds__(SP_T) void speckle_count_kernel(SpeckleArgs a) {
  const unsigned A = (unsigned)a.W * (unsigned)a.H, p = blockIdx.x * SP_T + threadIdx.x;
  if (p >= A) return;
  const size_t base = (size_t)blockIdx.y * A;
  unsigned* cnt = a.count + base;
  // nonzero exactly at the tile-local roots.  A root of the image may see its own word mid-sum: it only tests it against 0, and
  // the word was nonzero before this launch and only grows
  const unsigned c = cnt[p];
  if (c == 0) return;
  const unsigned* L = a.label + base;
  const unsigned r = uf_find(L, p);
  if (r != p) __hip_atomic_fetch_add(&cnt[r], c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // nobody adds to cnt[p]: p is no root
}

__global__ __launch_bounds__(SP_T) void speckle_apply_kernel(SpeckleArgs a) {
  __shared__ int sW[SP_T / 64];
  const unsigned A = (unsigned)a.W * (unsigned)a.H, p = blockIdx.x * SP_T + threadIdx.x;
  const size_t base = (size_t)blockIdx.y * A;
  int removed = 0;
  if (p < A) {
    const unsigned* L = a.label + base;
    const unsigned l = L[p];
    if (l != SP_NONE && a.count[base + uf_find(L, l)] <= (unsigned)a.max_size) {
      a.disp[base + p] = (int16_t)SP_FILTERED;
      removed = 1;
    }
  }
  if (!a.n_removed) return;
  for (int off = 32; off > 0; off >>= 1) removed += __shfl_xor(removed, off);
  if ((threadIdx.x & 63) == 0) sW[threadIdx.x >> 6] = removed;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
    for (int w = 0; w < SP_T / 64; ++w) t += sW[w];
    if (t) __hip_atomic_fetch_add(&a.n_removed[blockIdx.y], t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ----------------------------------------------------------------------------- host side
extern "C" size_t svo_speckle_workspace_bytes(int width, int height, int batch) { return speckle_workspace_bytes(width, height, batch); }

int svo_k_speckle(svo_ctx* ctx, int16_t* disp16, int batch, int W, int H, const svo_speckle_params* prm, void* workspace, int* n_removed) {
  if (prm->max_size == 0) return SVO_OK;  // no component has 0 pixels: the identity, and no launch
  const size_t A = (size_t)W * (size_t)H;
  SpeckleArgs a{};
  a.disp = disp16;
  a.label = static_cast<unsigned*>(workspace);
  a.count = a.label + A * (size_t)batch;
  a.n_removed = n_removed;
  const SpeckleGrid g = speckle_grid(W, H);
  a.W = W; a.H = H; a.tiles_x = g.tiles_x;
  a.max_size = prm->max_size; a.max_diff = prm->max_diff16;
  a.n_vert = g.n_vert; a.n_seam = g.n_seam;
  SvoProfScope prof(ctx, SVO_PROF_SPECKLE);
  hipLaunchKernelGGL(speckle_tile_kernel, dim3((unsigned)g.tiles_x * (unsigned)g.tiles_y, batch), dim3(SP_T), 0, ctx->stream, a);
  if (a.n_seam) hipLaunchKernelGGL(speckle_seam_kernel, dim3((a.n_seam + SP_T - 1) / SP_T, batch), dim3(SP_T), 0, ctx->stream, a);
  hipLaunchKernelGGL(speckle_count_kernel, dim3(g.px_blocks, batch), dim3(SP_T), 0, ctx->stream, a);
  hipLaunchKernelGGL(speckle_apply_kernel, dim3(g.px_blocks, batch), dim3(SP_T), 0, ctx->stream, a);
  SVO_HIP_CHECK(ctx, hipGetLastError());
  return SVO_OK;
}

extern "C" int svo_disparity_speckle_filter_batch_dev(svo_ctx* ctx, int16_t* disp16, int batch, int width, int height,
                                                      const svo_speckle_params* params, void* workspace, size_t workspace_bytes,
                                                      int* n_removed) {
  if (!ctx) return SVO_ERR_INVALID;
  svo_use_device(ctx);
  SVO_REQUIRE(ctx, disp16, "speckle_filter: null disp16");
  SVO_ARGS_CHECK(ctx, speckle_check(width, height, batch, params, &err));
  if (params->max_size == 0) return SVO_OK;
  SVO_REQUIRE(ctx, workspace && ((uintptr_t)workspace & 3) == 0, "speckle_filter: workspace is null or not 4-byte aligned");
  SVO_REQUIRE(ctx, workspace_bytes >= svo_speckle_workspace_bytes(width, height, batch),
              "speckle_filter: workspace_bytes is smaller than svo_speckle_workspace_bytes(width, height, batch)");
  return svo_k_speckle(ctx, disp16, batch, width, height, params, workspace, n_removed);
}

extern "C" int svo_disparity_speckle_filter(svo_ctx* ctx, int16_t* disp16, int width, int height, const svo_speckle_params* params,
                                            int* n_removed) {
  if (!ctx) return SVO_ERR_INVALID;
  svo_use_device(ctx);
  SVO_REQUIRE(ctx, disp16, "speckle_filter: null disp16");
  SVO_ARGS_CHECK(ctx, speckle_check(width, height, 1, params, &err));
  if (n_removed) *n_removed = 0;
  if (params->max_size == 0) return SVO_OK;
  SvoScratch s(ctx);
  const size_t px = (size_t)width * (size_t)height;
  int16_t* dD = s.take<int16_t>(px);
  int* dN = s.take<int>(1);
  unsigned* dW = s.take<unsigned>(2 * px);
  if (!dD || !dN || !dW) { ctx->err = "speckle_filter: the context's workspace is too small for this map (svo_limits.max_width / max_height)"; return SVO_ERR_CAPACITY; }
  hipStream_t st = ctx->stream;
  SVO_HIP_CHECK(ctx, hipMemcpyAsync(dD, disp16, px * sizeof(int16_t), hipMemcpyHostToDevice, st));
  const int rc = svo_k_speckle(ctx, dD, 1, width, height, params, dW, dN);
  if (rc) return rc;
  SVO_HIP_CHECK(ctx, hipMemcpyAsync(disp16, dD, px * sizeof(int16_t), hipMemcpyDeviceToHost, st));
  int n = 0;
  SVO_HIP_CHECK(ctx, hipMemcpyAsync(&n, dN, sizeof(int), hipMemcpyDeviceToHost, st));
  SVO_HIP_CHECK(ctx, hipStreamSynchronize(st));
  if (n_removed) *n_removed = n;
  return SVO_OK;
}
