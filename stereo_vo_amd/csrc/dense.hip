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
// each pass reads what the PREVIOUS launch of the same stream wrote.  The argument rules, the chunk counts and the LDS sizes are
// host/dense_args.h's; the keyframe clouds of a pipeline that call in here are host/keyframe_clouds.cpp.
#include "kernels.h"
#include "ref_constants.h"
#include "stereo_common.h"
#include "tail_device.h"

namespace {
constexpr int RAW_H = DT_TH + 2;                      // raw tile rows (halo 1)
constexpr int RAW_LP = (DT_TWL + 2 + 3) & ~3;         // raw left tile pitch (88)
constexpr int RAW_RP = (DT_TWR + 2 + 3) & ~3;         // raw right tile pitch (152)
static_assert(RAW_H * (RAW_LP + RAW_RP) <= (int)sizeof(unsigned short) * (16 + 1) * DT_PIX, "the raw tiles must fit the smallest SAD region (16 disparities)");

constexpr int CL_T = 256, CL_ITEMS = 8;  // threads and candidates per thread of a workgroup of the count / write passes
static_assert(CL_T * CL_ITEMS == CL_CHUNK, "a workgroup takes one chunk");

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
  const size_t sad_lds = dense_sad_lds(ndisp);
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

int svo_k_cloud(svo_ctx* ctx, const int16_t* disp16, const SvoDensePairs& src, int batch, int W, int H, int stride,
                const svo_camera_info* cam, const float* pose16, const svo_cloud_params* prm, svo_cloud_point* points, int* counts,
                int* seg) {
  SvoCloudArgs a{};
  a.disp = disp16; a.src = src; a.W = W; a.H = H; a.stride = stride;
  a.step = prm->step; a.nx = cloud_nx(W, prm->step); a.n_cand = cloud_n_cand(W, H, prm->step);
  a.n_chunks = cloud_chunks(W, H, prm->step);
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

extern "C" int svo_cloud_default_params(svo_cloud_params* p, int width, int height) { return cloud_default_params(p, width, height); }

// The plain and the cost form of the batched dense entry: `t` tells them apart (t.null_cost: the cost map is required).
static int stereo_bm_batch(svo_ctx* ctx, const uint8_t* left, const uint8_t* right, int batch, int width, int height, int row_stride,
                           size_t image_stride, int num_disparities, int block_size, int16_t* disp16, uint16_t* cost16, const DenseBatchTexts& t) {
  int rc = svo_stereo_check(ctx, left, right, width, height, row_stride, num_disparities, block_size);
  if (rc) return rc;
  SVO_REQUIRE(ctx, disp16, t.null_disp);
  if (t.null_cost) SVO_REQUIRE(ctx, cost16, t.null_cost);
  SVO_ARGS_CHECK(ctx, dense_batch_check(batch, ctx->lim.max_batch, width, height, row_stride, image_stride, t, &err));
  SvoDensePairs src{left, right, image_stride, nullptr};
  return svo_k_stereo_dense_batch(ctx, src, batch, width, height, row_stride, num_disparities, block_size, disp16, cost16);
}

extern "C" int svo_stereo_bm_batch_dev(svo_ctx* ctx, const uint8_t* left, const uint8_t* right, int batch, int width, int height,
                                       int row_stride, size_t image_stride, int num_disparities, int block_size, int16_t* disp16) {
  return stereo_bm_batch(ctx, left, right, batch, width, height, row_stride, image_stride, num_disparities, block_size, disp16, nullptr,
                         STEREO_BM_BATCH_TEXTS);
}

extern "C" int svo_stereo_bm_cost_batch_dev(svo_ctx* ctx, const uint8_t* left, const uint8_t* right, int batch, int width, int height,
                                            int row_stride, size_t image_stride, int num_disparities, int block_size, int16_t* disp16,
                                            uint16_t* cost16) {
  return stereo_bm_batch(ctx, left, right, batch, width, height, row_stride, image_stride, num_disparities, block_size, disp16, cost16,
                         STEREO_BM_COST_BATCH_TEXTS);
}

extern "C" int svo_disparity_cloud_batch_dev(svo_ctx* ctx, const int16_t* disp16, const uint8_t* left, int batch, int width, int height,
                                             int row_stride, size_t image_stride, const svo_camera_info* cam, const float* pose16,
                                             const svo_cloud_params* params, svo_cloud_point* points, int* counts) {
  if (!ctx) return SVO_ERR_INVALID;
  svo_use_device(ctx);
  SVO_REQUIRE(ctx, disp16 && left && points && counts, "disparity_cloud: null buffer");
  SVO_ARGS_CHECK(ctx, cloud_check(width, height, row_stride, cam, params, ctx->lim.max_width, ctx->lim.max_height, &err));
  SVO_REQUIRE(ctx, batch >= 1 && batch <= ctx->lim.max_batch, "disparity_cloud: batch outside 1..max_batch");
  // per-chunk counts for the largest call this context takes, once
  const size_t need = (size_t)ctx->lim.max_batch * (size_t)cloud_chunks(ctx->lim.max_width, ctx->lim.max_height, 1);
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
  SVO_ARGS_CHECK(ctx, cloud_check(width, height, row_stride, cam, params, ctx->lim.max_width, ctx->lim.max_height, &err));
  SvoScratch s(ctx);
  const size_t px = (size_t)width * height;
  uint8_t* dL = s.take<uint8_t>(px);
  uint8_t* dR = s.take<uint8_t>(px);
  int16_t* dD = s.take<int16_t>(px);
  float* dP = s.take<float>(16);
  int* dC = s.take<int>(2);
  int* dS = s.take<int>((size_t)cloud_chunks(width, height, params->step));
  const size_t cap = cloud_store_cap(params->max_points, px);
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
