// Left-right consistency check of CV_16S disparity maps (include/svo.h, "left-right check"): what `disp12MaxDiff` of
// StereoBM switches on, from the map and the winner's SAD per pixel, for a batch of maps in ONE launch on the context's stream.
//
//   lr_check_kernel : one workgroup per (row, map).  The row's values are copied to LDS; every non-FILTERED x votes for the
//                     right-view column x2 = x - ((d + 8) >> 4) with an LDS atomicMin of (cost << 16) | x on key[x2], so the
//                     column's winner is the lowest cost and, among equal costs, the smallest x, whatever order the votes
//                     arrive in.  After one barrier every x looks its two columns up, in LDS only (the winner's d is
//                     row[key & 0xFFFF], the LDS copy: the in-place store of FILTERED is never read back), and the removed
//                     pixels are summed per wavefront, per workgroup, and added to n_removed[map] with one atomicAdd.
//
// Rows are independent, so nothing passes between workgroups except that order-independent relaxed atomicAdd (docs/HISTORY.md,
// "No cache maintenance inside kernels"): no fence, no acquire / release, no waiting.  The LDS is 6 * W bytes (4 for the key, 2
// for the value), which fits the 64 KB every kernel gets without asking up to SVO_LR_CHECK_MAX_WIDTH; a key whose cost is 0xFFFF
// cannot equal the empty key 0xFFFFFFFF because x < 0xFFFF at that width.  Votes of adjacent x go to adjacent columns except at
// disparity steps, so the atomics of a wavefront fall on distinct banks except where pixels truly collide.
#include "dense_args.h"
#include "kernels.h"

namespace {
constexpr int LR_T = 256;
constexpr int LR_FILTERED = -16;
constexpr unsigned LR_EMPTY = 0xFFFFFFFFu;
static_assert(SVO_LR_CHECK_MAX_WIDTH < 0xFFFF, "x must not reach 0xFFFF: (0xFFFF << 16) | x would be the empty key");

struct LrCheckArgs {
  int16_t* disp;         // batch tight maps, checked in place
  const uint16_t* cost;  // batch tight maps
  int* n_removed;        // batch (zeroed on the stream before the launch), or null
  int W, H, max_diff;
};
}  // namespace

__global__ __launch_bounds__(LR_T) void lr_check_kernel(LrCheckArgs a) {
  extern __shared__ __align__(16) unsigned lr_lds[];  // key[W], then row[W]
  __shared__ int sW[LR_T / 64];
  unsigned* const key = lr_lds;
  short* const row = reinterpret_cast<short*>(lr_lds + a.W);
  const int W = a.W, tid = threadIdx.x;
  const size_t base = ((size_t)blockIdx.y * (size_t)a.H + (size_t)blockIdx.x) * (size_t)W;
  int16_t* __restrict__ disp = a.disp + base;
  const uint16_t* __restrict__ cost = a.cost + base;
  for (int x = tid; x < W; x += LR_T) {
    row[x] = disp[x];
    key[x] = LR_EMPTY;
  }
  __syncthreads();
  for (int x = tid; x < W; x += LR_T) {
    const int d = row[x];
    if (d == LR_FILTERED) continue;
    const int x2 = x - ((d + 8) >> 4);
    if (x2 >= 0 && x2 < W)
      __hip_atomic_fetch_min(&key[x2], ((unsigned)cost[x] << 16) | (unsigned)x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  __syncthreads();
  int removed = 0;
  for (int x = tid; x < W; x += LR_T) {
    const int d = row[x];
    if (d == LR_FILTERED) continue;
    auto bad = [&](int xq) -> bool {
      if (xq < 0 || xq >= W) return false;
      const unsigned k = key[xq];
      return k != LR_EMPTY && abs((int)row[k & 0xFFFFu] - d) > a.max_diff;  // int32: at most 65,535
    };
    if (bad(x - (d >> 4)) && bad(x - ((d + 15) >> 4))) {
      disp[x] = (int16_t)LR_FILTERED;
      ++removed;
    }
  }
  if (!a.n_removed) return;
  for (int off = 32; off > 0; off >>= 1) removed += __shfl_xor(removed, off);
  if ((tid & 63) == 0) sW[tid >> 6] = removed;
  __syncthreads();
  if (tid == 0) {
    int t = 0;
    for (int w = 0; w < LR_T / 64; ++w) t += sW[w];
    if (t) __hip_atomic_fetch_add(&a.n_removed[blockIdx.y], t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ----------------------------------------------------------------------------- host side
int svo_k_lr_check(svo_ctx* ctx, int16_t* disp16, const uint16_t* cost16, int batch, int W, int H, const svo_lr_check_params* prm,
                   int* n_removed) {
  LrCheckArgs a{};
  a.disp = disp16; a.cost = cost16; a.n_removed = n_removed;
  a.W = W; a.H = H; a.max_diff = prm->max_diff16;
  SvoProfScope prof(ctx, SVO_PROF_LR_CHECK);
  if (n_removed) SVO_HIP_CHECK(ctx, hipMemsetAsync(n_removed, 0, sizeof(int) * (size_t)batch, ctx->stream));
  hipLaunchKernelGGL(lr_check_kernel, dim3((unsigned)H, (unsigned)batch), dim3(LR_T), lr_check_lds(W), ctx->stream, a);
  SVO_HIP_CHECK(ctx, hipGetLastError());
  return SVO_OK;
}

extern "C" int svo_disparity_lr_check_batch_dev(svo_ctx* ctx, int16_t* disp16, const uint16_t* cost16, int batch, int width, int height,
                                                const svo_lr_check_params* params, int* n_removed) {
  if (!ctx) return SVO_ERR_INVALID;
  svo_use_device(ctx);
  SVO_REQUIRE(ctx, disp16, "lr_check: null disp16");
  SVO_REQUIRE(ctx, cost16, "lr_check: null cost16");
  SVO_ARGS_CHECK(ctx, lr_check_check(width, height, batch, params, &err));
  return svo_k_lr_check(ctx, disp16, cost16, batch, width, height, params, n_removed);
}

extern "C" int svo_disparity_lr_check(svo_ctx* ctx, int16_t* disp16, const uint16_t* cost16, int width, int height,
                                      const svo_lr_check_params* params, int* n_removed) {
  if (!ctx) return SVO_ERR_INVALID;
  svo_use_device(ctx);
  SVO_REQUIRE(ctx, disp16, "lr_check: null disp16");
  SVO_REQUIRE(ctx, cost16, "lr_check: null cost16");
  SVO_ARGS_CHECK(ctx, lr_check_check(width, height, 1, params, &err));
  SvoScratch s(ctx);
  const size_t px = (size_t)width * (size_t)height;
  int16_t* dD = s.take<int16_t>(px);
  uint16_t* dC = s.take<uint16_t>(px);
  int* dN = s.take<int>(1);
  if (!dD || !dC || !dN) { ctx->err = "lr_check: the context's workspace is too small for this map (svo_limits.max_width / max_height)"; return SVO_ERR_CAPACITY; }
  hipStream_t st = ctx->stream;
  SVO_HIP_CHECK(ctx, hipMemcpyAsync(dD, disp16, px * sizeof(int16_t), hipMemcpyHostToDevice, st));
  SVO_HIP_CHECK(ctx, hipMemcpyAsync(dC, cost16, px * sizeof(uint16_t), hipMemcpyHostToDevice, st));
  const int rc = svo_k_lr_check(ctx, dD, dC, 1, width, height, params, dN);
  if (rc) return rc;
  SVO_HIP_CHECK(ctx, hipMemcpyAsync(disp16, dD, px * sizeof(int16_t), hipMemcpyDeviceToHost, st));
  int n = 0;
  SVO_HIP_CHECK(ctx, hipMemcpyAsync(&n, dN, sizeof(int), hipMemcpyDeviceToHost, st));
  SVO_HIP_CHECK(ctx, hipStreamSynchronize(st));
  if (n_removed) *n_removed = n;
  return SVO_OK;
}
