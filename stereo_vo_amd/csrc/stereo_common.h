// What the sparse / dense block matchers of stereo.hip and the batched dense matcher of dense.hip share: StereoBM's constants
// (src/image_processor.cpp:173-176), the X-Sobel prefilter and the tile geometry of the dense kernels.
#ifndef SVO_STEREO_COMMON_H_
#define SVO_STEREO_COMMON_H_
#include "common.h"

namespace {
constexpr int CAP = 31, TEXTURE_THRESHOLD = 10, UNIQUENESS_RATIO = 15;
constexpr int MAX_NDISP = 64, MAX_BLOCK = 21;

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

// Dense kernels: workgroup = 64 columns x 8 rows of output (see stereo_dense_kernel).
namespace {
constexpr int DT_W = 64, DT_H = 8, DT_PIX = DT_W * DT_H;
constexpr int DT_TH = DT_H + MAX_BLOCK - 1;         // 28 tile rows
constexpr int DT_TWL = DT_W + MAX_BLOCK - 1;        // 84 left tile columns
constexpr int DT_TWR = DT_TWL + MAX_NDISP;          // right tile columns
constexpr int DT_SLOTS = 3;                         // disparity slots per pass
}

// argument limits of every StereoBM entry point (stereo.hip)
int svo_stereo_check(svo_ctx* ctx, const void* l, const void* r, int W, int H, int stride, int ndisp, int block);
#endif  // SVO_STEREO_COMMON_H_
