// The rectification table (include/svo.h "rectification"): where in the RAW image every pixel of the rectified image comes
// from, in 1/32 pixel.  The reference carries the coefficients (k1, k2, p1, p2 of CameraInfo, src/camera_info.hpp:10-14) and
// never reads them (src/vo_node.cpp:110 passes zeros); this is where they mean something.
//
// Declared arithmetic: everything is f64, every operation is rounded separately (the build passes -ffp-contract=off), and
// only + - x / and rint (ties to even) occur, so a plain float64 restatement gives the same bits.  For destination pixel
// (u, v), rectified camera (focal, cx, cy), raw camera (fx, fy, cx_raw, cy_raw, k1, k2, p1, p2, R), in this order:
//   xn = (u - cx) / focal,  yn = (v - cy) / focal
//   X = (R[0] xn + R[3] yn) + R[6],  Y = (R[1] xn + R[4] yn) + R[7],  W = (R[2] xn + R[5] yn) + R[8]      (R^T [xn yn 1]^T)
//   x = X / W,  y = Y / W
//   x2 = x x,  y2 = y y,  r2 = x2 + y2,  t = (2 x) y
//   kr = (k2 r2 + k1) r2 + 1
//   xd = (x kr + p1 t) + p2 (r2 + 2 x2),  yd = (y kr + p1 (r2 + 2 y2)) + p2 t
//   sx = fx xd + cx_raw,  sy = fy yd + cy_raw
//   qx = rint(32 sx),  qy = rint(32 sy)
// which is the construction of OpenCV's initUndistortRectifyMap followed by its 1/32-pixel fixed-point maps.
// Record: int16 dx = qx - 32 u, dy = qy - 32 v (a displacement, so that it fits 4 bytes at any image width).
// No source — the record (-32768, -32768) — when W <= 0 (or NaN), when 32 sx or 32 sy is not finite (or beyond 2^40 in
// magnitude: far outside any image), or when all four bilinear taps (qx >> 5, qx >> 5 + 1) x (qy >> 5, qy >> 5 + 1) lie
// outside the raw image.  A source with a tap inside whose displacement leaves [-32767, 32767] is an error, never clipped.
#include <math.h>
#include <stdio.h>

#include <string>

#include "kernels.h"

namespace {
thread_local std::string g_rect_err;
}

const char* svo_rectify_error_text() { return g_rect_err.c_str(); }

extern "C" int svo_rectify_eye_from_camera_info(const svo_camera_info* cam, svo_rectify_eye* eye) {
  if (!cam || !eye) return SVO_ERR_INVALID;
  eye->fx = eye->fy = cam->focal;
  eye->cx = cam->cx; eye->cy = cam->cy;
  eye->k1 = cam->k1; eye->k2 = cam->k2; eye->p1 = cam->p1; eye->p2 = cam->p2;
  for (int i = 0; i < 9; ++i) eye->R[i] = (i % 4 == 0) ? 1.0 : 0.0;
  return SVO_OK;
}

extern "C" int svo_rectify_build_map(const svo_rectify_eye* eye, const svo_camera_info* cam, int width, int height, int16_t* dxdy) {
  g_rect_err.clear();
  if (!eye || !cam || !dxdy) { g_rect_err = "rectify_build_map: null argument"; return SVO_ERR_INVALID; }
  if (width < 1 || height < 1 || width > 32767 || height > 32767) { g_rect_err = "rectify_build_map: image size outside 1..32767"; return SVO_ERR_INVALID; }
  if (!(cam->focal > 0.0) || !isfinite(cam->focal) || !isfinite(cam->cx) || !isfinite(cam->cy)) {
    g_rect_err = "rectify_build_map: the rectified camera needs a finite focal > 0 and a finite centre";
    return SVO_ERR_INVALID;
  }
  const double focal = cam->focal, cx = cam->cx, cy = cam->cy;
  const double fx = eye->fx, fy = eye->fy, cxr = eye->cx, cyr = eye->cy;
  const double k1 = eye->k1, k2 = eye->k2, p1 = eye->p1, p2 = eye->p2;
  const double* R = eye->R;
  const double far = 1099511627776.0;  // 2^40
  for (int v = 0; v < height; ++v) {
    const double yn = ((double)v - cy) / focal;
    for (int u = 0; u < width; ++u) {
      int16_t* rec = dxdy + 2 * ((size_t)v * width + u);
      rec[0] = rec[1] = (int16_t)-32768;
      const double xn = ((double)u - cx) / focal;
      const double X = (R[0] * xn + R[3] * yn) + R[6];
      const double Y = (R[1] * xn + R[4] * yn) + R[7];
      const double W = (R[2] * xn + R[5] * yn) + R[8];
      if (!(W > 0.0)) continue;
      const double x = X / W, y = Y / W;
      const double x2 = x * x, y2 = y * y, r2 = x2 + y2, t = (2.0 * x) * y;
      const double kr = (k2 * r2 + k1) * r2 + 1.0;
      const double xd = (x * kr + p1 * t) + p2 * (r2 + 2.0 * x2);
      const double yd = (y * kr + p1 * (r2 + 2.0 * y2)) + p2 * t;
      const double sx = fx * xd + cxr, sy = fy * yd + cyr;
      const double ex = 32.0 * sx, ey = 32.0 * sy;
      if (!(fabs(ex) < far) || !(fabs(ey) < far)) continue;  // also catches NaN and infinities
      const long long qx = (long long)rint(ex), qy = (long long)rint(ey);
      const long long ix = qx >> 5, iy = qy >> 5;
      if (ix < -1 || ix > (long long)width - 1 || iy < -1 || iy > (long long)height - 1) continue;  // all four taps outside
      const long long dx = qx - 32LL * u, dy = qy - 32LL * v;
      if (dx < -32767 || dx > 32767 || dy < -32767 || dy > 32767) {
        char msg[256];
        snprintf(msg, sizeof(msg), "rectify_build_map: the displacement of pixel (%d, %d), (%lld, %lld) / 32 px, does not fit an int16 "
                 "(at most 32767 / 32 px); the table is never clipped", u, v, dx, dy);
        g_rect_err = msg;
        return SVO_ERR_INVALID;
      }
      rec[0] = (int16_t)dx; rec[1] = (int16_t)dy;
    }
  }
  return SVO_OK;
}
