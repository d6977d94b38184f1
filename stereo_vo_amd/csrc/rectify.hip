// Rectification of raw stereo pairs: the table-driven warp in front of the pipeline (include/svo.h "rectification").
//
// The table comes from host/rectify.cpp (f64, declared operation order): one int32 record per destination pixel, dx in the
// low and dy in the high half, both in 1/32 pixel relative to the pixel itself; SVO_RECT_SENTINEL = no source.
//
// rectify_remap_kernel — bilinear interpolation in exact integers.  For a record (dx, dy) of pixel (u, v):
//   qx = 32 u + dx, ix = qx >> 5 (arithmetic), ax = qx & 31, and the same in y;
//   out = ((32-ax)(32-ay) p(ix,iy) + ax (32-ay) p(ix+1,iy) + (32-ax) ay p(ix,iy+1) + ax ay p(ix+1,iy+1) + 512) >> 10,
//   a tap outside the raw image contributes 0, a pixel without source is 0.
// Intent: these are the integers OpenCV's fixed-point INTER_LINEAR remap with a constant-0 border forms (its 15-bit
// weight table is these weights times 32, its rounding (. + 2^14) >> 15); the tests pin the arithmetic above, not OpenCV.
//
// Shape: ONE launch for every image of a call, blockIdx.z = (lane, frame, eye); the lane's tables come from a pointer
// table in the kernel arguments.  A thread owns a run of 4 consecutive destination pixels of one row, placed so that the
// run's first output byte is 4-byte aligned: one 16-byte load of the table (when the table address is aligned too: always
// for images whose size is a multiple of 4 bytes, else four 4-byte loads), 16 byte gathers from the raw image through
// the caches (a wavefront covers 256 consecutive pixels of a row: its taps are two short row segments, and the four
// rows of a workgroup share them), one 4-byte store.  Runs cut by the ends of a row, records without source and taps
// beyond the border take the checked path; a wavefront that meets none of them never branches into it.
// No LDS, no atomics, no fences, nothing shared between workgroups (the rule of docs/HISTORY.md "No cache maintenance
// inside kernels").
#include "kernels.h"

static_assert(SVO_RECT_MAX_LANES <= 255, "lane indices travel as bytes");

namespace {

constexpr int RECT_RUN = 4;     // destination pixels per thread
constexpr int RECT_TX = 64;     // threads along a row: one wavefront = 256 consecutive pixels
constexpr int RECT_TY = 4;      // rows per workgroup

__device__ __forceinline__ unsigned rect_blend(unsigned p00, unsigned p01, unsigned p10, unsigned p11, int ax, int ay) {
  const unsigned bx = 32u - (unsigned)ax, by = 32u - (unsigned)ay;
  return (bx * by * p00 + (unsigned)ax * by * p01 + bx * (unsigned)ay * p10 + (unsigned)ax * (unsigned)ay * p11 + 512u) >> 10;
}

__global__ __launch_bounds__(RECT_TX* RECT_TY) void rectify_remap_kernel(const SvoRectifyArgs a) {
  const int z = blockIdx.z;
  const int e = z % a.eyes, kf = z / a.eyes;
  const int f = kf % a.frames, k = kf / a.frames;
  const int W = a.width, H = a.height;
  const int v = blockIdx.y * RECT_TY + threadIdx.y;
  if (v >= H) return;
  const size_t lane = a.lane[k];
  const uint8_t* __restrict__ src = a.src[e] + lane * a.src_lane_stride + (size_t)f * a.src_image_stride;
  uint8_t* __restrict__ drow = a.dst[e] + lane * a.dst_lane_stride + (size_t)f * a.dst_image_stride + (size_t)v * W;
  const int* __restrict__ mrow = a.map[k][e] + (size_t)v * W;
  const int stride = a.src_row_stride;
  // runs start where the output is 4-byte aligned: the row's first run is cut short by `head` pixels
  const int head = (int)(reinterpret_cast<uintptr_t>(drow) & 3u);
  const int u0 = RECT_RUN * (int)(blockIdx.x * RECT_TX + threadIdx.x) - head;
  if (u0 >= W) return;
  const bool full = u0 >= 0 && u0 + RECT_RUN <= W;

  int rec[RECT_RUN];
  if (full && (reinterpret_cast<uintptr_t>(mrow + u0) & 15u) == 0) {
    const int4 r4 = *reinterpret_cast<const int4*>(mrow + u0);
    rec[0] = r4.x; rec[1] = r4.y; rec[2] = r4.z; rec[3] = r4.w;
  } else {
#pragma unroll
    for (int j = 0; j < RECT_RUN; ++j) rec[j] = (unsigned)(u0 + j) < (unsigned)W ? mrow[u0 + j] : SVO_RECT_SENTINEL;
  }

  int ix[RECT_RUN], iy[RECT_RUN], ax[RECT_RUN], ay[RECT_RUN];
  bool inside = full;
#pragma unroll
  for (int j = 0; j < RECT_RUN; ++j) {
    const int qx = 32 * (u0 + j) + (int)(short)(rec[j] & 0xffff);
    const int qy = 32 * v + (rec[j] >> 16);
    ix[j] = qx >> 5; ax[j] = qx & 31;
    iy[j] = qy >> 5; ay[j] = qy & 31;
    inside = inside && rec[j] != SVO_RECT_SENTINEL && ix[j] >= 0 && ix[j] + 1 < W && iy[j] >= 0 && iy[j] + 1 < H;
  }

  if (inside) {  // all 16 taps lie in the raw image
    unsigned p[RECT_RUN][4];
#pragma unroll
    for (int j = 0; j < RECT_RUN; ++j) {
      const uint8_t* q = src + (size_t)iy[j] * stride + ix[j];
      p[j][0] = q[0]; p[j][1] = q[1]; p[j][2] = q[stride]; p[j][3] = q[stride + 1];
    }
    unsigned out = 0;
#pragma unroll
    for (int j = 0; j < RECT_RUN; ++j) out |= rect_blend(p[j][0], p[j][1], p[j][2], p[j][3], ax[j], ay[j]) << (8 * j);
    *reinterpret_cast<unsigned*>(drow + u0) = out;
    return;
  }

  // checked path: the ends of a row, records without source, taps beyond the border
  unsigned out = 0;
#pragma unroll
  for (int j = 0; j < RECT_RUN; ++j) {
    unsigned val = 0;
    if (rec[j] != SVO_RECT_SENTINEL) {
      const bool x0 = (unsigned)ix[j] < (unsigned)W, x1 = (unsigned)(ix[j] + 1) < (unsigned)W;
      const bool y0 = (unsigned)iy[j] < (unsigned)H, y1 = (unsigned)(iy[j] + 1) < (unsigned)H;
      const uint8_t* q = src + (ptrdiff_t)iy[j] * stride + ix[j];
      const unsigned p00 = (x0 && y0) ? q[0] : 0u, p01 = (x1 && y0) ? q[1] : 0u;
      const unsigned p10 = (x0 && y1) ? q[stride] : 0u, p11 = (x1 && y1) ? q[stride + 1] : 0u;
      val = rect_blend(p00, p01, p10, p11, ax[j], ay[j]);
    }
    out |= val << (8 * j);
  }
  if (full) {
    *reinterpret_cast<unsigned*>(drow + u0) = out;
  } else {
#pragma unroll
    for (int j = 0; j < RECT_RUN; ++j)
      if ((unsigned)(u0 + j) < (unsigned)W) drow[u0 + j] = (uint8_t)(out >> (8 * j));
  }
}

}  // namespace

int svo_k_rectify_remap(svo_ctx* ctx, const SvoRectifyArgs& a, hipStream_t st) {
  SVO_REQUIRE(ctx, a.width >= 1 && a.height >= 1 && a.src_row_stride >= a.width && a.frames >= 1 && (a.eyes == 1 || a.eyes == 2) &&
                       a.n_active >= 1 && a.n_active <= SVO_RECT_MAX_LANES, "rectify_remap: bad launch shape");
  const size_t images = (size_t)a.n_active * (size_t)a.frames * (size_t)a.eyes;
  SVO_REQUIRE(ctx, images <= 65535, "rectify_remap: more than 65535 images in one launch");
  const int runs = (a.width + 3 + RECT_RUN - 1) / RECT_RUN;  // a row's first run may be cut short by up to 3 pixels
  const dim3 grid((unsigned)svo_div_up(runs, RECT_TX), (unsigned)svo_div_up(a.height, RECT_TY), (unsigned)images);
  SvoProfScope prof(ctx, SVO_PROF_RECTIFY, st);
  hipLaunchKernelGGL(rectify_remap_kernel, grid, dim3(RECT_TX, RECT_TY, 1), 0, st, a);
  SVO_HIP_CHECK(ctx, hipGetLastError());
  return SVO_OK;
}

// ---- the tables of one camera in HBM
int svo_rect_model_create(svo_ctx* ctx, const svo_rectify_eye* left, const svo_rectify_eye* right, const svo_camera_info* cam,
                          int width, int height, SvoRectModel** out) {
  if (!ctx || !left || !cam || !out) return SVO_ERR_INVALID;
  *out = nullptr;
  SVO_REQUIRE(ctx, width >= 1 && height >= 1 && width <= 32767 && height <= 32767, "rectification: image size outside 1..32767");
  const size_t n = (size_t)width * height;
  std::vector<int16_t> h(2 * n);
  SvoRectModel* m = new SvoRectModel();
  const svo_rectify_eye* eyes[2] = {left, right};
  for (int e = 0; e < 2; ++e) {
    if (!eyes[e]) continue;
    m->eye[e] = *eyes[e];
    int rc = svo_rectify_build_map(eyes[e], cam, width, height, h.data());
    if (rc) { ctx->err = std::string(e ? "right eye: " : "left eye: ") + svo_rectify_error_text(); svo_rect_model_destroy(m); return rc; }
    hipError_t he = hipMalloc((void**)&m->d_map[e], sizeof(int) * n);
    if (he == hipSuccess) he = hipMemcpy(m->d_map[e], h.data(), sizeof(int) * n, hipMemcpyHostToDevice);
    if (he != hipSuccess) {
      ctx->err = std::string("rectification: table upload failed: ") + hipGetErrorString(he);
      svo_rect_model_destroy(m);
      return SVO_ERR_HIP;
    }
  }
  *out = m;
  return SVO_OK;
}

void svo_rect_model_destroy(SvoRectModel* m) {
  if (!m) return;
  for (int e = 0; e < 2; ++e) if (m->d_map[e]) (void)hipFree(m->d_map[e]);
  delete m;
}

// ---- C-ABI: stand-alone use
extern "C" int svo_rectify_remap_batch_dev(svo_ctx* ctx, const uint8_t* raw, int batch, int width, int height, int row_stride,
                                           size_t image_stride, const svo_rectify_eye* eye, const svo_camera_info* cam, uint8_t* out) {
  if (!ctx) return SVO_ERR_INVALID;
  svo_use_device(ctx);
  SVO_REQUIRE(ctx, raw && out && eye && cam, "rectify_remap: null argument");
  SVO_REQUIRE(ctx, batch >= 1 && batch <= 65535 && width >= 1 && height >= 1 && row_stride >= width &&
                       image_stride >= (size_t)row_stride * (size_t)(height - 1) + (size_t)width, "rectify_remap: bad shape");
  SvoRectModel* m = nullptr;
  int rc = svo_rect_model_create(ctx, eye, nullptr, cam, width, height, &m);
  if (rc) return rc;
  SvoRectifyArgs a{};
  a.src[0] = raw; a.dst[0] = out;
  a.src_image_stride = image_stride; a.dst_image_stride = (size_t)width * height;
  a.src_row_stride = row_stride; a.width = width; a.height = height; a.frames = batch; a.eyes = 1; a.n_active = 1;
  a.map[0][0] = m->d_map[0]; a.lane[0] = 0;
  rc = svo_k_rectify_remap(ctx, a, ctx->stream);
  // the table is this call's own: it must outlive the launch
  if (hipStreamSynchronize(ctx->stream) != hipSuccess && !rc) { ctx->err = "rectify_remap: launch failed"; rc = SVO_ERR_HIP; }
  svo_rect_model_destroy(m);
  return rc;
}

extern "C" int svo_rectify_remap(svo_ctx* ctx, const uint8_t* raw, int width, int height, int row_stride, const svo_rectify_eye* eye,
                                 const svo_camera_info* cam, uint8_t* out) {
  if (!ctx) return SVO_ERR_INVALID;
  svo_use_device(ctx);
  SVO_REQUIRE(ctx, raw && out && eye && cam, "rectify_remap: null argument");
  SVO_REQUIRE(ctx, width >= 1 && height >= 1 && row_stride >= width && width <= ctx->lim.max_width && height <= ctx->lim.max_height,
              "rectify_remap: image size outside limits");
  const size_t bytes = (size_t)width * height;
  SvoScratch s(ctx);
  uint8_t* d_raw = s.take<uint8_t>(bytes);
  uint8_t* d_out = s.take<uint8_t>(bytes);
  if (!d_raw || !d_out) { ctx->err = "rectify_remap: workspace too small"; return SVO_ERR_CAPACITY; }
  SVO_HIP_CHECK(ctx, hipMemcpy2DAsync(d_raw, width, raw, row_stride, width, height, hipMemcpyHostToDevice, ctx->stream));
  const int rc = svo_rectify_remap_batch_dev(ctx, d_raw, 1, width, height, width, bytes, eye, cam, d_out);
  if (rc) return rc;
  SVO_HIP_CHECK(ctx, hipMemcpy(out, d_out, bytes, hipMemcpyDeviceToHost));
  return SVO_OK;
}
