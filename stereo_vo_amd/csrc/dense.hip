// Dense keyframe depth: batched StereoBM maps and compacted point clouds (include/svo.h, "dense depth clouds").
// The dense form of src/image_processor.cpp:173-207: the whole CV_16S map of StereoBM::compute (:174-175) for a batch of pairs
// in one launch, then one 3-D point per kept pixel with the arithmetic of the per-feature loop (:178-207).
//
//   stereo_dense_batch_kernel : stereo_dense_kernel (stereo.hip) with blockIdx.z = pair, reading the RAW images: the raw tile
//                               with a one-pixel halo is staged in LDS, the X-Sobel prefilter (prefilter_at) of the left and
//                               right tiles is formed there; no prefiltered image exists in HBM.  The raw tiles live in the
//                               region that holds the SADs afterwards, so the LDS footprint is that of stereo_dense_kernel.
//   cloud_count / cloud_scan / cloud_write : raster order without one workgroup ever waiting for another means counting
//                               first: kept pixels per chunk of 2048 candidates, an exclusive scan per image by one
//                               workgroup, then the write pass recomputes the predicate and compacts inside its chunk.
// No kernel here has a fence, cache maintenance or an ordered atomic (docs/HISTORY.md, "No cache maintenance inside kernels"):
// each pass reads what the PREVIOUS launch of the same stream wrote.
#include <new>

#include "kernels.h"
#include "ref_constants.h"
#include "stereo_common.h"
#include "tail_device.h"

namespace {
constexpr int RAW_H = DT_TH + 2;                      // raw tile rows (halo 1)
constexpr int RAW_LP = (DT_TWL + 2 + 3) & ~3;         // raw left tile pitch (88)
constexpr int RAW_RP = (DT_TWR + 2 + 3) & ~3;         // raw right tile pitch (152)
constexpr int DENSE_LDS_MAX = (int)sizeof(unsigned short) * (MAX_NDISP + 1) * DT_PIX;  // 66,560 B
static_assert(RAW_H * (RAW_LP + RAW_RP) <= (int)sizeof(unsigned short) * (16 + 1) * DT_PIX, "the raw tiles must fit the smallest SAD region (16 disparities)");

constexpr int CL_T = 256, CL_ITEMS = 8, CL_CHUNK = CL_T * CL_ITEMS;  // candidates per workgroup of the count / write passes

__device__ __forceinline__ const uint8_t* pair_image(const SvoDensePairs& s, int z, int eye) {
  if (s.tab) return eye ? s.tab[z].right : s.tab[z].left;
  return (eye ? s.right : s.left) + (size_t)z * s.image_stride;
}
}  // namespace

// COST: the cost form (svo_stereo_bm_cost_batch_dev, the keyframe maps when the left-right check is on), which also writes the
// winner's SAD of the selection loop, cost[y][x] (0xFFFF where the map is FILTERED; minsad <= 21 * 21 * 62 = 27,342 never collides).
// Without COST nothing of it is compiled and `cost` is never read: the plain instantiation is the kernel as it was before the cost
// form existed, and it is what every plain path launches.
template <bool COST>
__global__ __launch_bounds__(256) void stereo_dense_batch_kernel(SvoDensePairs src, int W, int H, int stride, int ndisp, int block,
                                                                 int16_t* __restrict__ out, uint16_t* __restrict__ cost) {
  __shared__ uint8_t sL[DT_TH][DT_TWL + 4], sR[DT_TH][DT_TWR + 4];
  __shared__ unsigned short sV[DT_SLOTS][DT_H][DT_TWL + 4];
  extern __shared__ __align__(16) unsigned short sSad[];  // [ndisp + 1][DT_PIX]; before the first SAD is written: the raw tiles
  uint8_t* const rawL = reinterpret_cast<uint8_t*>(sSad);
  uint8_t* const rawR = rawL + RAW_H * RAW_LP;
  const uint8_t* __restrict__ L = pair_image(src, blockIdx.z, 0);
  const uint8_t* __restrict__ R = pair_image(src, blockIdx.z, 1);
  out += (size_t)blockIdx.z * W * H;
  if (COST) cost += (size_t)blockIdx.z * W * H;
  const int half = block / 2;
  const int x0 = blockIdx.x * DT_W, y0 = blockIdx.y * DT_H;
  const int tid = threadIdx.x;
  const int th = DT_H + block - 1, twl = DT_W + block - 1, twr = twl + ndisp - 1;
  // ---- raw tiles with halo 1, coordinates clamped into the image (a clamped value is only ever read for a pixel whose prefilter
  // does not depend on it: prefilter_at tests the borders itself)
  const int ry0 = y0 - half - 1, rlx0 = x0 - half - 1, rrx0 = x0 - half - (ndisp - 1) - 1;
  for (int i = tid; i < (th + 2) * (twl + 2); i += 256) {
    const int r = i / (twl + 2), c = i % (twl + 2);
    rawL[r * RAW_LP + c] = L[(size_t)min(max(ry0 + r, 0), H - 1) * stride + min(max(rlx0 + c, 0), W - 1)];
  }
  for (int i = tid; i < (th + 2) * (twr + 2); i += 256) {
    const int r = i / (twr + 2), c = i % (twr + 2);
    rawR[r * RAW_RP + c] = R[(size_t)min(max(ry0 + r, 0), H - 1) * stride + min(max(rrx0 + c, 0), W - 1)];
  }
  __syncthreads();
  // ---- prefiltered tiles (0 outside the image, as stereo_dense_kernel reads them)
  auto IL = [&](int xx, int yy) -> int { return rawL[(yy - ry0) * RAW_LP + (xx - rlx0)]; };
  auto IR = [&](int xx, int yy) -> int { return rawR[(yy - ry0) * RAW_RP + (xx - rrx0)]; };
  for (int i = tid; i < th * twl; i += 256) {
    const int r = i / twl, c = i % twl;
    const int gx = x0 - half + c, gy = y0 - half + r;
    sL[r][c] = (gx >= 0 && gx < W && gy >= 0 && gy < H) ? (uint8_t)prefilter_at(IL, gx, gy, W, H) : 0;
  }
  for (int i = tid; i < th * twr; i += 256) {
    const int r = i / twr, c = i % twr;
    const int gx = x0 - half - (ndisp - 1) + c, gy = y0 - half + r;
    sR[r][c] = (gx >= 0 && gx < W && gy >= 0 && gy < H) ? (uint8_t)prefilter_at(IR, gx, gy, W, H) : 0;
  }
  __syncthreads();  // the raw tiles are dead from here on: sSad is written after the next barrier
  const int nslots = ndisp + 1;
  const int vs = tid / DT_TWL, vc = tid % DT_TWL;   // vertical pass: slot-in-pass, tile column (tid < 252 active)
  for (int s0 = 0; s0 < nslots; s0 += DT_SLOTS) {
    // ---- vertical running sums
    if (vs < DT_SLOTS && vc < twl && s0 + vs < nslots) {
      const int slot = s0 + vs;
      const bool tex = slot == ndisp;
      auto AD = [&](int r) -> int {
        const int l = sL[r][vc];
        return tex ? abs(l - CAP) : abs(l - (int)sR[r][vc + slot]);
      };
      int sum = 0;
      for (int r = 0; r < block; ++r) sum += AD(r);
      sV[vs][0][vc] = (unsigned short)sum;
      for (int r = 1; r < DT_H; ++r) {
        sum += AD(r + block - 1) - AD(r - 1);
        sV[vs][r][vc] = (unsigned short)sum;
      }
    }
    __syncthreads();
    // ---- horizontal sums: work item = (slot-in-pass, row, group of 4 adjacent outputs)
    for (int item = tid; item < DT_SLOTS * DT_H * (DT_W / 4); item += 256) {
      const int hs = item / (DT_H * (DT_W / 4)), rem = item % (DT_H * (DT_W / 4));
      const int r = rem / (DT_W / 4), xg = (rem % (DT_W / 4)) * 4;
      if (s0 + hs >= nslots) continue;
      const unsigned short* v = &sV[hs][r][xg];
      int h0 = 0;
      for (int c = 0; c < block; ++c) h0 += v[c];
      const int h1 = h0 - v[0] + v[block], h2 = h1 - v[1] + v[block + 1], h3 = h2 - v[2] + v[block + 2];
      unsigned short* o = &sSad[(size_t)(s0 + hs) * DT_PIX + r * DT_W + xg];
      o[0] = (unsigned short)h0; o[1] = (unsigned short)h1; o[2] = (unsigned short)h2; o[3] = (unsigned short)h3;
    }
    __syncthreads();
  }
  // ---- selection (StereoBM winner, uniqueness, texture, sub-pixel): two pixels per thread
  for (int pix = tid; pix < DT_PIX; pix += 256) {
    const int x = x0 + (pix % DT_W), y = y0 + pix / DT_W;
    if (x >= W || y >= H) continue;
    int res = -16, won = 0xFFFF;
    if (x >= ndisp - 1 + half && x < W - half && y >= half && y < H - half) {
      auto S = [&](int i) -> int { return sSad[(size_t)i * DT_PIX + pix]; };
      const int tsum = S(ndisp);
      if (tsum >= TEXTURE_THRESHOLD) {
        int minsad = 0x7fffffff, mind = -1;
        for (int i = 0; i < ndisp; ++i) {
          const int v = S(i);
          if (v < minsad) { minsad = v; mind = i; }
        }
        const int thresh = minsad + (minsad * UNIQUENESS_RATIO / 100);
        bool unique = true;
        for (int i = 0; i < ndisp && unique; ++i)
          if ((i < mind - 1 || i > mind + 1) && S(i) <= thresh) unique = false;
        if (unique) {
          // borders as bm_select: s[-1] = s[1], s[ndisp] = s[ndisp - 2]
          const int p = mind + 1 < ndisp ? S(mind + 1) : S(ndisp - 2);
          const int n = mind - 1 >= 0 ? S(mind - 1) : S(1);
          const int dd = p + n - 2 * minsad + abs(p - n);
          res = (short)(((ndisp - mind - 1) * 256 + (dd != 0 ? (p - n) * 256 / dd : 0) + 15) >> 4);  // >= -8: never FILTERED
          won = minsad;
        }
      }
    }
    out[(size_t)y * W + x] = (int16_t)res;
    if (COST) cost[(size_t)y * W + x] = (uint16_t)won;
  }
}

// ----------------------------------------------------------------------------- clouds
// Candidate k of an image (raster order over the pixels with x % step == 0 and y % step == 0): its pixel, and whether it is kept
// (src/image_processor.cpp:176 convertTo(CV_32F, 1/16), :194 the test, with the caller's lower bound).
struct SvoCloudArgs {
  const int16_t* disp;  // batch tight maps
  SvoDensePairs src;    // the left images (tag only)
  int W, H, stride;
  int step, nx, n_cand, n_chunks;
  float thr;            // max(min_disparity, 0)
  int max_points;
  SvoMat4 Q;            // the reprojection matrix of the camera (svo_k_reprojection_q)
  const float* pose16;  // batch x 16 or null (identity)
  svo_cloud_point* points;
  int* counts;          // batch x {n_total, n_stored}
  int* seg;             // batch x n_chunks: kept per chunk, then (after the scan) kept before the chunk
};

namespace {
__device__ __forceinline__ bool cloud_keep(const SvoCloudArgs& a, const int16_t* __restrict__ disp, int k, int& x, int& y, float& d) {
  if (k >= a.n_cand) return false;
  const int yy = k / a.nx, xx = k - yy * a.nx;
  x = xx * a.step; y = yy * a.step;
  d = (float)disp[(size_t)y * a.W + x] * svo_ref::STEREO_DISPARITY_SCALE;
  return d > a.thr;
}
}  // namespace

__global__ __launch_bounds__(CL_T) void cloud_count_kernel(SvoCloudArgs a) {
  __shared__ int sW[CL_T / 64];
  const int b = blockIdx.y, chunk = blockIdx.x;
  const int16_t* __restrict__ disp = a.disp + (size_t)b * a.W * a.H;
  int cnt = 0;
#pragma unroll
  for (int j = 0; j < CL_ITEMS; ++j) {
    int x, y; float d;
    cnt += cloud_keep(a, disp, chunk * CL_CHUNK + j * CL_T + (int)threadIdx.x, x, y, d) ? 1 : 0;
  }
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
  if ((threadIdx.x & 63) == 0) sW[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
    for (int w = 0; w < CL_T / 64; ++w) t += sW[w];
    a.seg[(size_t)b * a.n_chunks + chunk] = t;
  }
}

// One workgroup per image: seg[] (kept per chunk) -> kept before the chunk, and the image's two counts.
__global__ __launch_bounds__(CL_T) void cloud_scan_kernel(SvoCloudArgs a) {
  __shared__ int sW[CL_T / 64];
  const int b = blockIdx.x;
  int* seg = a.seg + (size_t)b * a.n_chunks;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int carry = 0;
  for (int c0 = 0; c0 < a.n_chunks; c0 += CL_T) {
    const int c = c0 + (int)threadIdx.x;
    const int v = c < a.n_chunks ? seg[c] : 0;
    int inc = v;
    for (int off = 1; off < 64; off <<= 1) {
      const int t = __shfl_up(inc, off);
      if (lane >= off) inc += t;
    }
    if (lane == 63) sW[wave] = inc;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < CL_T / 64; ++w) {
      const int t = sW[w];
      if (w < wave) before += t;
      total += t;
    }
    if (c < a.n_chunks) seg[c] = carry + before + inc - v;
    carry += total;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    a.counts[2 * b] = carry;
    a.counts[2 * b + 1] = min(carry, a.max_points);
  }
}

__global__ __launch_bounds__(CL_T) void cloud_write_kernel(SvoCloudArgs a) {
  __shared__ int sW[CL_T / 64];
  __shared__ SvoMat4 sM;
  const int b = blockIdx.y, chunk = blockIdx.x;
  int base = a.seg[(size_t)b * a.n_chunks + chunk];
  if (base >= a.max_points) return;  // workgroup-uniform: everything from here on is past the stored part
  // M = pose * Q as svo_k_reprojection_matrix forms it: f64 products summed in order, rounded to f32
  if (threadIdx.x < 16) {
    const int i = threadIdx.x >> 2, j = threadIdx.x & 3;
    double s = 0.0;
    for (int k = 0; k < 4; ++k) {
      const float p = a.pose16 ? a.pose16[16 * (size_t)b + 4 * i + k] : (i == k ? 1.0f : 0.0f);
      s += (double)p * (double)a.Q.m[4 * k + j];
    }
    sM.m[threadIdx.x] = (float)s;
  }
  __syncthreads();
  const int16_t* __restrict__ disp = a.disp + (size_t)b * a.W * a.H;
  const uint8_t* __restrict__ left = pair_image(a.src, b, 0);
  svo_cloud_point* __restrict__ out = a.points + (size_t)b * a.max_points;
  for (int j = 0; j < CL_ITEMS; ++j) {
    int x = 0, y = 0; float d = 0.f;
    const bool keep = cloud_keep(a, disp, chunk * CL_CHUNK + j * CL_T + (int)threadIdx.x, x, y, d);
    const int slot = svo_compact_slot<CL_T>(keep, base, sW);
    if (slot >= 0 && slot < a.max_points) {
      float p[3];
      svo_triangulate_point(sM, (float)x, (float)y, d, p);
      svo_cloud_point q;
      q.x = p[0]; q.y = p[1]; q.z = p[2];
      q.tag = (uint32_t)(y * a.W + x) | ((uint32_t)left[(size_t)y * a.stride + x] << 24);
      out[slot] = q;
    }
  }
}

// ----------------------------------------------------------------------------- host side
int svo_k_stereo_dense_batch(svo_ctx* ctx, const SvoDensePairs& src, int batch, int W, int H, int stride, int ndisp, int block,
                             int16_t* disp16, uint16_t* cost16) {
  const size_t sad_lds = sizeof(unsigned short) * (size_t)(ndisp + 1) * DT_PIX;
  // the grant belongs to the device the kernel was loaded on, and to ONE kernel function (hipFuncSetAttribute is per function):
  // remembered per context (= per device) and per form, not per process
  int& granted = cost16 ? ctx->dense_cost_lds_granted : ctx->dense_lds_granted;
  auto* const kernel = cost16 ? stereo_dense_batch_kernel<true> : stereo_dense_batch_kernel<false>;
  if ((int)sad_lds > granted) {
    SVO_HIP_CHECK(ctx, hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, DENSE_LDS_MAX));
    granted = DENSE_LDS_MAX;
  }
  SvoProfScope prof(ctx, SVO_PROF_STEREO_DENSE_BATCH);
  hipLaunchKernelGGL(kernel, dim3(svo_div_up(W, DT_W), svo_div_up(H, DT_H), batch), dim3(256), sad_lds, ctx->stream,
                     src, W, H, stride, ndisp, block, disp16, cost16);
  SVO_HIP_CHECK(ctx, hipGetLastError());
  return SVO_OK;
}

int svo_k_cloud_chunks(int W, int H, int step) {
  const long n = (long)svo_div_up(W, step) * svo_div_up(H, step);
  return (int)((n + CL_CHUNK - 1) / CL_CHUNK);
}

int svo_k_cloud(svo_ctx* ctx, const int16_t* disp16, const SvoDensePairs& src, int batch, int W, int H, int stride,
                const svo_camera_info* cam, const float* pose16, const svo_cloud_params* prm, svo_cloud_point* points, int* counts,
                int* seg) {
  SvoCloudArgs a{};
  a.disp = disp16; a.src = src; a.W = W; a.H = H; a.stride = stride;
  a.step = prm->step; a.nx = svo_div_up(W, prm->step); a.n_cand = a.nx * svo_div_up(H, prm->step);
  a.n_chunks = svo_k_cloud_chunks(W, H, prm->step);
  a.thr = prm->min_disparity > 0.f ? prm->min_disparity : 0.f;
  a.max_points = prm->max_points;
  a.Q = svo_k_reprojection_q((float)cam->focal, (float)cam->cx, (float)cam->cy, (float)cam->baseline);
  a.pose16 = pose16; a.points = points; a.counts = counts; a.seg = seg;
  SvoProfScope prof(ctx, SVO_PROF_CLOUD);
  hipLaunchKernelGGL(cloud_count_kernel, dim3(a.n_chunks, batch), dim3(CL_T), 0, ctx->stream, a);
  hipLaunchKernelGGL(cloud_scan_kernel, dim3(batch), dim3(CL_T), 0, ctx->stream, a);
  hipLaunchKernelGGL(cloud_write_kernel, dim3(a.n_chunks, batch), dim3(CL_T), 0, ctx->stream, a);
  SVO_HIP_CHECK(ctx, hipGetLastError());
  return SVO_OK;
}

static int cloud_check(svo_ctx* ctx, int W, int H, int stride, const svo_camera_info* cam, const svo_cloud_params* prm) {
  SVO_REQUIRE(ctx, cam && prm, "cloud: null camera or parameters");
  SVO_REQUIRE(ctx, W >= 1 && H >= 1 && (long)W * (long)H <= (1L << 24), "cloud: width*height must be at most 2^24 (the tag holds the pixel index in 24 bits)");
  SVO_REQUIRE(ctx, W <= ctx->lim.max_width && H <= ctx->lim.max_height && stride >= W, "cloud: image size outside limits");
  SVO_REQUIRE(ctx, prm->step >= 1, "cloud: step must be at least 1");
  SVO_REQUIRE(ctx, prm->max_points >= 1, "cloud: max_points must be at least 1");
  SVO_REQUIRE(ctx, cam->focal != 0.0 && cam->baseline != 0.0, "cloud: focal length and baseline must not be 0");
  return SVO_OK;
}

extern "C" int svo_cloud_default_params(svo_cloud_params* p, int width, int height) {
  if (!p || width < 1 || height < 1 || (long)width * (long)height > (1L << 24)) return SVO_ERR_INVALID;
  p->step = 1;
  p->min_disparity = 0.f;
  p->max_points = width * height;
  return SVO_OK;
}

extern "C" int svo_stereo_bm_batch_dev(svo_ctx* ctx, const uint8_t* left, const uint8_t* right, int batch, int width, int height,
                                       int row_stride, size_t image_stride, int num_disparities, int block_size, int16_t* disp16) {
  int rc = svo_stereo_check(ctx, left, right, width, height, row_stride, num_disparities, block_size);
  if (rc) return rc;
  SVO_REQUIRE(ctx, disp16, "stereo_bm_batch: null output");
  SVO_REQUIRE(ctx, batch >= 1 && batch <= ctx->lim.max_batch, "stereo_bm_batch: batch outside 1..max_batch");
  SVO_REQUIRE(ctx, batch == 1 || image_stride >= (size_t)row_stride * (size_t)(height - 1) + (size_t)width, "stereo_bm_batch: images overlap");
  SvoDensePairs src{left, right, image_stride, nullptr};
  return svo_k_stereo_dense_batch(ctx, src, batch, width, height, row_stride, num_disparities, block_size, disp16);
}

extern "C" int svo_stereo_bm_cost_batch_dev(svo_ctx* ctx, const uint8_t* left, const uint8_t* right, int batch, int width, int height,
                                            int row_stride, size_t image_stride, int num_disparities, int block_size, int16_t* disp16,
                                            uint16_t* cost16) {
  int rc = svo_stereo_check(ctx, left, right, width, height, row_stride, num_disparities, block_size);
  if (rc) return rc;
  SVO_REQUIRE(ctx, disp16, "stereo_bm_cost_batch: null disp16");
  SVO_REQUIRE(ctx, cost16, "stereo_bm_cost_batch: null cost16");
  SVO_REQUIRE(ctx, batch >= 1 && batch <= ctx->lim.max_batch, "stereo_bm_cost_batch: batch outside 1..max_batch");
  SVO_REQUIRE(ctx, batch == 1 || image_stride >= (size_t)row_stride * (size_t)(height - 1) + (size_t)width, "stereo_bm_cost_batch: images overlap");
  SvoDensePairs src{left, right, image_stride, nullptr};
  return svo_k_stereo_dense_batch(ctx, src, batch, width, height, row_stride, num_disparities, block_size, disp16, cost16);
}

extern "C" int svo_disparity_cloud_batch_dev(svo_ctx* ctx, const int16_t* disp16, const uint8_t* left, int batch, int width, int height,
                                             int row_stride, size_t image_stride, const svo_camera_info* cam, const float* pose16,
                                             const svo_cloud_params* params, svo_cloud_point* points, int* counts) {
  if (!ctx) return SVO_ERR_INVALID;
  svo_use_device(ctx);
  SVO_REQUIRE(ctx, disp16 && left && points && counts, "disparity_cloud: null buffer");
  int rc = cloud_check(ctx, width, height, row_stride, cam, params);
  if (rc) return rc;
  SVO_REQUIRE(ctx, batch >= 1 && batch <= ctx->lim.max_batch, "disparity_cloud: batch outside 1..max_batch");
  // per-chunk counts for the largest call this context takes, once
  const size_t need = (size_t)ctx->lim.max_batch * (size_t)svo_k_cloud_chunks(ctx->lim.max_width, ctx->lim.max_height, 1);
  if (ctx->cloud_seg_ints < need) {
    SVO_HIP_CHECK(ctx, hipMalloc((void**)&ctx->d_cloud_seg, need * sizeof(int)));
    ctx->cloud_seg_ints = need;
  }
  SvoDensePairs src{left, nullptr, image_stride, nullptr};
  return svo_k_cloud(ctx, disp16, src, batch, width, height, row_stride, cam, pose16, params, points, counts, ctx->d_cloud_seg);
}

extern "C" int svo_stereo_cloud(svo_ctx* ctx, const uint8_t* left, const uint8_t* right, int width, int height, int row_stride,
                                int num_disparities, int block_size, const svo_camera_info* cam, const float* pose16,
                                const svo_cloud_params* params, svo_cloud_point* points, int* n_total, int* n_stored) {
  int rc = svo_stereo_check(ctx, left, right, width, height, row_stride, num_disparities, block_size);
  if (rc) return rc;
  SVO_REQUIRE(ctx, points && n_total && n_stored, "stereo_cloud: null output");
  rc = cloud_check(ctx, width, height, row_stride, cam, params);
  if (rc) return rc;
  SvoScratch s(ctx);
  const size_t px = (size_t)width * height;
  uint8_t* dL = s.take<uint8_t>(px);
  uint8_t* dR = s.take<uint8_t>(px);
  int16_t* dD = s.take<int16_t>(px);
  float* dP = s.take<float>(16);
  int* dC = s.take<int>(2);
  int* dS = s.take<int>((size_t)svo_k_cloud_chunks(width, height, params->step));
  const size_t cap = (size_t)params->max_points < px ? (size_t)params->max_points : px;  // no more than px points exist
  svo_cloud_point* dQ = s.take<svo_cloud_point>(cap);
  if (!dL || !dR || !dD || !dP || !dC || !dS || !dQ) { ctx->err = "stereo_cloud: workspace too small"; return SVO_ERR_CAPACITY; }
  hipStream_t st = ctx->stream;
  SVO_HIP_CHECK(ctx, hipMemcpy2DAsync(dL, width, left, row_stride, width, height, hipMemcpyHostToDevice, st));
  SVO_HIP_CHECK(ctx, hipMemcpy2DAsync(dR, width, right, row_stride, width, height, hipMemcpyHostToDevice, st));
  if (pose16) SVO_HIP_CHECK(ctx, hipMemcpyAsync(dP, pose16, 16 * sizeof(float), hipMemcpyHostToDevice, st));
  SvoDensePairs src{dL, dR, px, nullptr};
  rc = svo_k_stereo_dense_batch(ctx, src, 1, width, height, width, num_disparities, block_size, dD);
  if (rc) return rc;
  svo_cloud_params prm = *params;
  prm.max_points = (int)cap;
  rc = svo_k_cloud(ctx, dD, src, 1, width, height, width, cam, pose16 ? dP : nullptr, &prm, dQ, dC, dS);
  if (rc) return rc;
  int c[2] = {0, 0};
  SVO_HIP_CHECK(ctx, hipMemcpyAsync(c, dC, sizeof(c), hipMemcpyDeviceToHost, st));
  SVO_HIP_CHECK(ctx, hipStreamSynchronize(st));
  *n_total = c[0]; *n_stored = c[1];
  if (c[1] > 0) {
    SVO_HIP_CHECK(ctx, hipMemcpyAsync(points, dQ, sizeof(svo_cloud_point) * (size_t)c[1], hipMemcpyDeviceToHost, st));
    SVO_HIP_CHECK(ctx, hipStreamSynchronize(st));
  }
  return SVO_OK;
}

// ----------------------------------------------------------------------------- keyframe clouds of a pipeline / a group
struct SvoKfClouds {
  svo_ctx* ctx = nullptr;
  svo_cloud_params prm{};
  int W = 0, H = 0, max_kf = 0;
  int16_t* d_disp = nullptr;          // max_kf maps
  svo_cloud_point* d_points = nullptr;  // max_kf x max_points
  int* d_counts = nullptr;            // max_kf x 2
  int* d_seg = nullptr;               // max_kf x chunks
  SvoCloudPair* d_tab = nullptr;      // max_kf
  void* h_pinned = nullptr;           // [max_kf pairs | max_kf x 2 counts]
  bool speckle_on = false;            // svo_kfc_set_speckle: the maps are filtered before the clouds are formed
  svo_speckle_params speckle{};
  void* d_speckle_ws = nullptr;       // svo_speckle_workspace_bytes(W, H, max_kf)
  bool lr_on = false;                 // svo_kfc_set_lr_check: the cost form of the dense launch, then the left-right check
  svo_lr_check_params lr{};
  uint16_t* d_cost = nullptr;         // max_kf cost maps, 2 * W * H * max_kf bytes
  bool sgm_on = false;                // svo_kfc_set_sgm: semi-global matching (sgm.hip) instead of the dense launch
  svo_sgm_params sgm{};
  void* d_sgm_ws = nullptr;           // svo_sgm_workspace_bytes for SVO_SGM_KEYFRAME_SUB_BATCH pairs, whatever max_kf is
  std::vector<svo_keyframe_cloud> table;
};

void svo_kfc_destroy(SvoKfClouds* k) {
  if (!k) return;
  (void)hipSetDevice(k->ctx->device);
  (void)hipStreamSynchronize(k->ctx->stream);
  void* ptrs[] = {k->d_disp, k->d_points, k->d_counts, k->d_seg, k->d_tab, k->d_speckle_ws, k->d_cost, k->d_sgm_ws};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  if (k->h_pinned) (void)hipHostFree(k->h_pinned);
  delete k;
}

int svo_kfc_create(svo_ctx* ctx, const svo_cloud_params* params, int W, int H, int max_kf, SvoKfClouds** out) {
  *out = nullptr;
  svo_use_device(ctx);
  svo_cloud_params prm = *params;
  SVO_REQUIRE(ctx, (long)W * (long)H <= (1L << 24), "set_keyframe_clouds: width*height must be at most 2^24");
  if (prm.max_points <= 0) prm.max_points = W * H;
  SVO_REQUIRE(ctx, prm.step >= 1, "set_keyframe_clouds: step must be at least 1");
  if (max_kf == 0) max_kf = ctx->lim.max_batch;
  SVO_REQUIRE(ctx, max_kf >= 1 && max_kf <= 65535, "set_keyframe_clouds: max_keyframes_per_call must be 0 or 1..65535");
  SvoKfClouds* k = new (std::nothrow) SvoKfClouds();
  if (!k) return SVO_ERR_HIP;
  k->ctx = ctx; k->prm = prm; k->W = W; k->H = H; k->max_kf = max_kf;
  const size_t px = (size_t)W * H, n = (size_t)max_kf;
  hipError_t e = hipMalloc((void**)&k->d_disp, n * px * sizeof(int16_t));
  if (e == hipSuccess) e = hipMalloc((void**)&k->d_points, n * (size_t)prm.max_points * sizeof(svo_cloud_point));
  if (e == hipSuccess) e = hipMalloc((void**)&k->d_counts, n * 2 * sizeof(int));
  if (e == hipSuccess) e = hipMalloc((void**)&k->d_seg, n * (size_t)svo_k_cloud_chunks(W, H, prm.step) * sizeof(int));
  if (e == hipSuccess) e = hipMalloc((void**)&k->d_tab, n * sizeof(SvoCloudPair));
  if (e == hipSuccess) e = hipHostMalloc(&k->h_pinned, n * (sizeof(SvoCloudPair) + 2 * sizeof(int)), hipHostMallocDefault);
  if (e != hipSuccess) {
    ctx->err = std::string("set_keyframe_clouds: allocation failed: ") + hipGetErrorString(e);
    svo_kfc_destroy(k);
    return SVO_ERR_HIP;
  }
  *out = k;
  return SVO_OK;
}

const svo_cloud_params* svo_kfc_params(const SvoKfClouds* k) { return &k->prm; }
int svo_kfc_max_keyframes(const SvoKfClouds* k) { return k->max_kf; }
void svo_kfc_clear(SvoKfClouds* k) { k->table.clear(); }
const svo_speckle_params* svo_kfc_speckle(const SvoKfClouds* k) { return k->speckle_on ? &k->speckle : nullptr; }

int svo_kfc_set_speckle(SvoKfClouds* k, const svo_speckle_params* prm) {
  svo_ctx* ctx = k->ctx;
  svo_use_device(ctx);
  if (!prm) {
    SVO_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    if (k->d_speckle_ws) (void)hipFree(k->d_speckle_ws);
    k->d_speckle_ws = nullptr;
    k->speckle_on = false;
    return SVO_OK;
  }
  const int rc = svo_speckle_check(ctx, k->W, k->H, k->max_kf, prm);
  if (rc) return rc;
  if (!k->d_speckle_ws) {
    const hipError_t e = hipMalloc(&k->d_speckle_ws, svo_speckle_workspace_bytes(k->W, k->H, k->max_kf));
    if (e != hipSuccess) {
      k->d_speckle_ws = nullptr;
      ctx->err = std::string("set_keyframe_speckle_filter: allocation failed: ") + hipGetErrorString(e);
      return SVO_ERR_HIP;
    }
  }
  k->speckle = *prm;
  k->speckle_on = true;
  return SVO_OK;
}

const svo_lr_check_params* svo_kfc_lr_check(const SvoKfClouds* k) { return k->lr_on ? &k->lr : nullptr; }

int svo_kfc_set_lr_check(SvoKfClouds* k, const svo_lr_check_params* prm) {
  svo_ctx* ctx = k->ctx;
  svo_use_device(ctx);
  if (!prm) {
    SVO_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    if (k->d_cost) (void)hipFree(k->d_cost);
    k->d_cost = nullptr;
    k->lr_on = false;
    return SVO_OK;
  }
  const int rc = svo_lr_check_check(ctx, k->W, k->H, k->max_kf, prm);
  if (rc) return rc;
  if (!k->d_cost) {
    const hipError_t e = hipMalloc((void**)&k->d_cost, sizeof(uint16_t) * (size_t)k->W * (size_t)k->H * (size_t)k->max_kf);
    if (e != hipSuccess) {
      k->d_cost = nullptr;
      ctx->err = std::string("set_keyframe_lr_check: allocation failed: ") + hipGetErrorString(e);
      return SVO_ERR_HIP;
    }
  }
  k->lr = *prm;
  k->lr_on = true;
  return SVO_OK;
}

const svo_sgm_params* svo_kfc_sgm(const SvoKfClouds* k) { return k->sgm_on ? &k->sgm : nullptr; }

int svo_kfc_set_sgm(SvoKfClouds* k, const svo_sgm_params* prm) {
  svo_ctx* ctx = k->ctx;
  svo_use_device(ctx);
  if (!prm) {
    SVO_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    if (k->d_sgm_ws) (void)hipFree(k->d_sgm_ws);
    k->d_sgm_ws = nullptr;
    k->sgm_on = false;
    return SVO_OK;
  }
  const int nd = svo_ref::STEREO_NUM_DISPARITIES, bs = svo_ref::STEREO_BLOCK_SIZE;
  const int rc = svo_sgm_check(ctx, k->W, k->H, nd, bs, SVO_SGM_KEYFRAME_SUB_BATCH, prm);
  if (rc) return rc;
  if (!k->d_sgm_ws) {
    const hipError_t e = hipMalloc(&k->d_sgm_ws, svo_sgm_workspace_bytes(k->W, k->H, nd, bs, SVO_SGM_KEYFRAME_SUB_BATCH));
    if (e != hipSuccess) {
      k->d_sgm_ws = nullptr;
      ctx->err = std::string("set_keyframe_sgm: allocation failed: ") + hipGetErrorString(e);
      return SVO_ERR_HIP;
    }
  }
  k->sgm = *prm;
  k->sgm_on = true;
  return SVO_OK;
}

int svo_kfc_run(SvoKfClouds* k, const svo_camera_info* cam, const SvoCloudPair* pairs, const int* frame, const int* lane, int n) {
  svo_ctx* ctx = k->ctx;
  k->table.clear();
  if (n <= 0) return SVO_OK;
  if (n > k->max_kf) {
    ctx->err = "keyframe clouds: " + std::to_string(n) + " keyframes in this call, max_keyframes_per_call is " + std::to_string(k->max_kf) +
               " (no cloud was produced; the frame results are complete)";
    return SVO_ERR_CAPACITY;
  }
  svo_cloud_params one{};
  one.step = 1; one.max_points = 1;
  int rc = cloud_check(ctx, k->W, k->H, k->W, cam, &one);
  if (rc) return rc;
  hipStream_t st = ctx->stream;
  SvoCloudPair* h_tab = static_cast<SvoCloudPair*>(k->h_pinned);
  int* h_counts = reinterpret_cast<int*>(h_tab + k->max_kf);
  memcpy(h_tab, pairs, sizeof(SvoCloudPair) * (size_t)n);
  SVO_HIP_CHECK(ctx, hipMemcpyAsync(k->d_tab, h_tab, sizeof(SvoCloudPair) * (size_t)n, hipMemcpyHostToDevice, st));
  SvoDensePairs src{nullptr, nullptr, 0, k->d_tab};
  if (k->sgm_on) {  // the matching sequence per sub-batch: the one workspace is reused, the launches are ordered by the stream
    const size_t px = (size_t)k->W * (size_t)k->H;
    for (int b0 = 0; b0 < n; b0 += SVO_SGM_KEYFRAME_SUB_BATCH) {
      const int nb = n - b0 < SVO_SGM_KEYFRAME_SUB_BATCH ? n - b0 : SVO_SGM_KEYFRAME_SUB_BATCH;
      SvoDensePairs sub{nullptr, nullptr, 0, k->d_tab + b0};
      rc = svo_k_stereo_sgm(ctx, sub, nb, k->W, k->H, k->W, svo_ref::STEREO_NUM_DISPARITIES, svo_ref::STEREO_BLOCK_SIZE, &k->sgm, k->d_sgm_ws,
                            k->d_disp + (size_t)b0 * px, k->lr_on ? k->d_cost + (size_t)b0 * px : nullptr);
      if (rc) return rc;
    }
  } else {
    rc = svo_k_stereo_dense_batch(ctx, src, n, k->W, k->H, k->W, svo_ref::STEREO_NUM_DISPARITIES, svo_ref::STEREO_BLOCK_SIZE, k->d_disp,
                                  k->lr_on ? k->d_cost : nullptr);
  }
  if (rc) return rc;
  if (k->lr_on) {  // same stream, before the speckle filter as in StereoBM::compute
    rc = svo_k_lr_check(ctx, k->d_disp, k->d_cost, n, k->W, k->H, &k->lr, nullptr);
    if (rc) return rc;
  }
  if (k->speckle_on) {  // same stream: the clouds below are those of the filtered maps
    rc = svo_k_speckle(ctx, k->d_disp, n, k->W, k->H, &k->speckle, k->d_speckle_ws, nullptr);
    if (rc) return rc;
  }
  rc = svo_k_cloud(ctx, k->d_disp, src, n, k->W, k->H, k->W, cam, nullptr, &k->prm, k->d_points, k->d_counts, k->d_seg);
  if (rc) return rc;
  SVO_HIP_CHECK(ctx, hipMemcpyAsync(h_counts, k->d_counts, sizeof(int) * 2 * (size_t)n, hipMemcpyDeviceToHost, st));
  SVO_HIP_CHECK(ctx, hipStreamSynchronize(st));
  k->table.resize((size_t)n);
  for (int i = 0; i < n; ++i) {
    svo_keyframe_cloud& t = k->table[(size_t)i];
    t.frame = frame[i]; t.lane = lane ? lane[i] : 0;
    t.n_total = h_counts[2 * i]; t.n_stored = h_counts[2 * i + 1];
    t.dev = k->d_points + (size_t)i * (size_t)k->prm.max_points;
  }
  return SVO_OK;
}

int svo_kfc_table(SvoKfClouds* k, int* n, const svo_keyframe_cloud** table) {
  *n = (int)k->table.size();
  if (table) *table = k->table.empty() ? nullptr : k->table.data();
  return SVO_OK;
}

int svo_kfc_copy(SvoKfClouds* k, int i, svo_cloud_point* host, int capacity) {
  svo_ctx* ctx = k->ctx;
  svo_use_device(ctx);
  SVO_REQUIRE(ctx, i >= 0 && i < (int)k->table.size() && capacity >= 0 && (host || capacity == 0), "copy_keyframe_cloud: no such entry, or null buffer");
  const int m = k->table[(size_t)i].n_stored < capacity ? k->table[(size_t)i].n_stored : capacity;
  if (m > 0) {
    SVO_HIP_CHECK(ctx, hipMemcpyAsync(host, k->table[(size_t)i].dev, sizeof(svo_cloud_point) * (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
    SVO_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  }
  return SVO_OK;
}

int svo_kfc_disparity(SvoKfClouds* k, int i, const int16_t** dev) {
  svo_ctx* ctx = k->ctx;
  SVO_REQUIRE(ctx, dev, "keyframe_disparity: null dev");
  *dev = nullptr;
  SVO_REQUIRE(ctx, i >= 0 && i < (int)k->table.size(), "keyframe_disparity: no such entry");
  *dev = k->d_disp + (size_t)i * (size_t)k->W * (size_t)k->H;
  return SVO_OK;
}

int svo_kfc_copy_disparity(SvoKfClouds* k, int i, int16_t* host) {
  svo_ctx* ctx = k->ctx;
  svo_use_device(ctx);
  SVO_REQUIRE(ctx, host, "copy_keyframe_disparity: null buffer");
  const int16_t* dev = nullptr;
  const int rc = svo_kfc_disparity(k, i, &dev);
  if (rc) return rc;
  SVO_HIP_CHECK(ctx, hipMemcpyAsync(host, dev, sizeof(int16_t) * (size_t)k->W * (size_t)k->H, hipMemcpyDeviceToHost, ctx->stream));
  SVO_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return SVO_OK;
}
