// What the sparse / dense block matchers of stereo.hip, the batched dense matcher of dense.hip and sgm.hip share: StereoBM's
// constants (src/image_processor.cpp:173-176) and the X-Sobel prefilter.  The limits MAX_NDISP / MAX_BLOCK and
// the tile geometry of the dense kernels (DT_*) are host/dense_args.h's, with the argument rules.
#ifndef SVO_STEREO_COMMON_H_
#define SVO_STEREO_COMMON_H_
#include "common.h"
#include "dense_args.h"

namespace {
constexpr int CAP = 31, TEXTURE_THRESHOLD = 10, UNIQUENESS_RATIO = 15;

__device__ __forceinline__ int pf_row(int y, int H) {
  if (y < 0) return H > 1 ? 1 : 0;
  if (y >= H) return H > 1 ? H - 2 : 0;
  return y;
}

// XSOBEL prefilter value at (x,y) from a raw image (global or LDS accessor).
template <typename Load>
__device__ __forceinline__ int prefilter_at(Load I, int x, int y, int W, int H) {
  if (x <= 0 || x >= W - 1) return CAP;
  if ((H & 1) && y == H - 1) return CAP;  // leftover odd row
  const int y0 = pf_row(y - 1, H), y2 = pf_row(y + 1, H);
  const int v = (I(x + 1, y0) - I(x - 1, y0)) + 2 * (I(x + 1, y) - I(x - 1, y)) + (I(x + 1, y2) - I(x - 1, y2));
  return min(max(v, -CAP), CAP) + CAP;
}
}  // namespace

// argument limits of every StereoBM entry point (stereo.hip): null context, device selection, then stereo_shape_check
int svo_stereo_check(svo_ctx* ctx, const void* l, const void* r, int W, int H, int stride, int ndisp, int block);
#endif  // SVO_STEREO_COMMON_H_
