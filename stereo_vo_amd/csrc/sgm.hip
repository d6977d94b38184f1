// Semi-global matching over StereoBM's cost volume (include/svo.h, "semi-global matching"): the project's own
// contract, exact integer arithmetic, no parity with OpenCV's SGBM claimed.
//
//   sgm_fill_kernel   : FILTERED / 0xFFFF over the whole of every map (the last path kernel overwrites the valid rectangle).
//   sgm_volume_kernel : the LDS tile of stereo_dense_batch_kernel (prefiltered tiles, vertical running sums, horizontal sums)
//                       over the VALID RECTANGLE only, written out instead of selected: C[pair][y][x][i] (u16, i = ndisp-1-d as
//                       StereoBM indexes its SADs) and the texture sum T[pair][y][x] (u16).  The prefilter is formed from the
//                       raw images with prefilter_at, as everywhere.
//   sgm_path_kernel<DIR, LPS> : one scanline per group of LPS lanes (16, 32 or 64; 48 disparities use 64 with 16 lanes idle), so
//                       a wavefront serves 4, 2 or 1 scanlines; lanes are disparities, min_k L(q, k) is a butterfly of
//                       __shfl_xor inside the group and L(q, d +- 1) a shift by one lane.  [y][x][i] makes every step of every
//                       direction one contiguous load of ndisp u16.  DIR 0 (left->right) stores S = L, DIR 1 (right->left) and
//                       DIR 2 (top->bottom) add to S, DIR 3 (bottom->top) adds in registers and selects: StereoBM's selection
//                       on S (first minimum in i, uniqueness, texture, sub-pixel), so S is read three times and written three.
//
// Nothing passes between workgroups of one launch: each launch reads what EARLIER launches of the same stream wrote (no fence,
// no acquire / release, no waiting; docs/HISTORY.md, "No cache maintenance inside kernels").  All offsets are 64-bit.
#include "kernels.h"
#include "ref_constants.h"
#include "stereo_common.h"

namespace {
constexpr int SGM_FILTERED = -16;
constexpr int SGM_BIG = 1 << 29;       // "no value": above every L (<= 60,109) and every S << 6 | i (< 2^24), + p1 / p2 stays in int32
constexpr int SGM_PF = 4;              // path steps whose loads are in flight ahead of the arithmetic

__device__ __forceinline__ const uint8_t* sgm_image(const SvoDensePairs& s, int z, int eye) {
  if (s.tab) return eye ? s.tab[z].right : s.tab[z].left;
  return (eye ? s.right : s.left) + (size_t)z * s.image_stride;
}

struct SgmArgs {
  SvoDensePairs src;
  int W, H, stride, ndisp, block;
  int rx0, ry0, VW, VH;  // the valid rectangle: origin and size
  int p1, p2;
  uint16_t* vol;   // batch x VH x VW x ndisp
  uint32_t* sum;   // the same count
  uint16_t* tex;   // batch x VH x VW
  int16_t* out;    // batch x H x W
  uint16_t* cost;  // batch x H x W or null
};
}  // namespace

__global__ __launch_bounds__(SGM_T) void sgm_fill_kernel(int16_t* __restrict__ out, uint16_t* __restrict__ cost, size_t n) {
  const size_t k = (size_t)blockIdx.x * SGM_T + threadIdx.x;
  if (k >= n) return;
  out[k] = (int16_t)SGM_FILTERED;
  if (cost) cost[k] = 0xFFFF;
}

// Workgroup = DT_W x DT_H pixels of the valid rectangle of pair blockIdx.z.
__global__ __launch_bounds__(SGM_T) void sgm_volume_kernel(SgmArgs a) {
  __shared__ uint8_t sL[DT_TH][DT_TWL + 4], sR[DT_TH][DT_TWR + 4];
  __shared__ unsigned short sV[DT_SLOTS][DT_H][DT_TWL + 4];
  extern __shared__ __align__(16) unsigned short sgm_sad[];  // [ndisp + 1][SGM_SP]
  const uint8_t* __restrict__ L = sgm_image(a.src, blockIdx.z, 0);
  const uint8_t* __restrict__ R = sgm_image(a.src, blockIdx.z, 1);
  const int W = a.W, H = a.H, ndisp = a.ndisp, block = a.block, half = block / 2, stride = a.stride;
  const int vx0 = blockIdx.x * DT_W, vy0 = blockIdx.y * DT_H;
  const int x0 = a.rx0 + vx0, y0 = a.ry0 + vy0;
  const int tid = threadIdx.x;
  const int th = DT_H + block - 1, twl = DT_W + block - 1, twr = twl + ndisp - 1;
  auto IL = [&](int xx, int yy) -> int { return L[(size_t)yy * stride + xx]; };
  auto IR = [&](int xx, int yy) -> int { return R[(size_t)yy * stride + xx]; };
  // ---- prefiltered tiles, 0 outside the image (prefilter_at reads inside the image only)
  for (int i = tid; i < th * twl; i += SGM_T) {
    const int r = i / twl, c = i % twl;
    const int gx = x0 - half + c, gy = y0 - half + r;
    sL[r][c] = (gx >= 0 && gx < W && gy >= 0 && gy < H) ? (uint8_t)prefilter_at(IL, gx, gy, W, H) : 0;
  }
  for (int i = tid; i < th * twr; i += SGM_T) {
    const int r = i / twr, c = i % twr;
    const int gx = x0 - half - (ndisp - 1) + c, gy = y0 - half + r;
    sR[r][c] = (gx >= 0 && gx < W && gy >= 0 && gy < H) ? (uint8_t)prefilter_at(IR, gx, gy, W, H) : 0;
  }
  __syncthreads();
  const int nslots = ndisp + 1;
  const int vs = tid / DT_TWL, vc = tid % DT_TWL;
  for (int s0 = 0; s0 < nslots; s0 += DT_SLOTS) {
    // ---- vertical running sums of |l - r| (slot ndisp: |l - CAP|, the texture sum)
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
    for (int item = tid; item < DT_SLOTS * DT_H * (DT_W / 4); item += SGM_T) {
      const int hs = item / (DT_H * (DT_W / 4)), rem = item % (DT_H * (DT_W / 4));
      const int r = rem / (DT_W / 4), xg = (rem % (DT_W / 4)) * 4;
      if (s0 + hs >= nslots) continue;
      const unsigned short* v = &sV[hs][r][xg];
      int h0 = 0;
      for (int c = 0; c < block; ++c) h0 += v[c];
      const int h1 = h0 - v[0] + v[block], h2 = h1 - v[1] + v[block + 1], h3 = h2 - v[2] + v[block + 2];
      unsigned short* o = &sgm_sad[(size_t)(s0 + hs) * SGM_SP + r * DT_W + xg];
      o[0] = (unsigned short)h0; o[1] = (unsigned short)h1; o[2] = (unsigned short)h2; o[3] = (unsigned short)h3;
    }
    __syncthreads();
  }
  // ---- write-out, i fastest: one tile row is DT_W * ndisp contiguous u16
  const size_t pair = (size_t)blockIdx.z * (size_t)a.VW * (size_t)a.VH;
  uint16_t* __restrict__ vol = a.vol + pair * (size_t)ndisp;
  uint16_t* __restrict__ tex = a.tex + pair;
  for (int idx = tid; idx < DT_PIX * ndisp; idx += SGM_T) {
    const int i = idx % ndisp, pix = idx / ndisp;
    const int vx = vx0 + pix % DT_W, vy = vy0 + pix / DT_W;
    if (vx < a.VW && vy < a.VH) vol[((size_t)vy * a.VW + vx) * (size_t)ndisp + i] = sgm_sad[(size_t)i * SGM_SP + pix];
  }
  for (int pix = tid; pix < DT_PIX; pix += SGM_T) {
    const int vx = vx0 + pix % DT_W, vy = vy0 + pix / DT_W;
    if (vx < a.VW && vy < a.VH) tex[(size_t)vy * a.VW + vx] = sgm_sad[(size_t)ndisp * SGM_SP + pix];
  }
}

template <int LPS>
__device__ __forceinline__ int sgm_group_min(int v) {
#pragma unroll
  for (int off = LPS / 2; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off));
  return v;
}

// DIR: 0 left->right (S = L), 1 right->left (S += L), 2 top->bottom (S += L), 3 bottom->top (S + L selected, nothing stored).
// Grid: x = groups of 4 wavefronts over the scanlines, y = pair.  Every lane of a wavefront runs every step (the shuffles need
// them); `live` guards the loads and stores alone.
template <int DIR, int LPS>
__global__ __launch_bounds__(SGM_T) void sgm_path_kernel(SgmArgs a) {
  constexpr int PER = 64 / LPS;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & (LPS - 1), sub = lane / LPS;
  const int ndisp = a.ndisp, VW = a.VW, VH = a.VH;
  const int nlines = DIR < 2 ? VH : VW, nsteps = DIR < 2 ? VW : VH;
  const int line0 = (blockIdx.x * (SGM_T / 64) + wave) * PER;
  if (line0 >= nlines) return;  // the whole wavefront
  const int line = line0 + sub;
  const bool lane_d = i < ndisp;
  const bool live = line < nlines && lane_d;
  const size_t pair = (size_t)blockIdx.y * (size_t)VW * (size_t)VH;
  const uint16_t* __restrict__ vol = a.vol + pair * (size_t)ndisp;
  uint32_t* __restrict__ sum = a.sum + pair * (size_t)ndisp;
  const uint16_t* __restrict__ tex = a.tex + pair;
  auto pixel = [&](int t) -> size_t {  // of step t of this lane's scanline, in the rectangle
    const int tt = (DIR & 1) ? nsteps - 1 - t : t;
    return DIR < 2 ? (size_t)line * VW + tt : (size_t)tt * VW + line;
  };
  int cbuf[SGM_PF], tbuf[SGM_PF];
  unsigned sbuf[SGM_PF];
  auto load = [&](int t, int k) {
    cbuf[k] = 0; sbuf[k] = 0; tbuf[k] = 0;
    if (live && t < nsteps) {
      const size_t px = pixel(t), off = px * (size_t)ndisp + i;
      cbuf[k] = vol[off];
      if (DIR > 0) sbuf[k] = sum[off];
      if (DIR == 3 && i == 0) tbuf[k] = tex[px];
    }
  };
#pragma unroll
  for (int k = 0; k < SGM_PF; ++k) load(k, k);
  int prev = SGM_BIG, pm = 0;
  for (int t0 = 0; t0 < nsteps; t0 += SGM_PF) {
    int cc[SGM_PF], tt[SGM_PF];
    unsigned ss[SGM_PF];
#pragma unroll
    for (int k = 0; k < SGM_PF; ++k) { cc[k] = cbuf[k]; ss[k] = sbuf[k]; tt[k] = tbuf[k]; }
#pragma unroll
    for (int k = 0; k < SGM_PF; ++k) load(t0 + SGM_PF + k, k);
#pragma unroll
    for (int k = 0; k < SGM_PF; ++k) {
      const int t = t0 + k;
      if (t >= nsteps) break;  // wavefront-uniform
      int Lr = cc[k];
      if (t > 0) {
        const int dn = __shfl(prev, lane - 1), up = __shfl(prev, lane + 1);
        int best = min(prev, pm + a.p2);
        if (i > 0) best = min(best, dn + a.p1);
        if (i < ndisp - 1) best = min(best, up + a.p1);
        Lr += best - pm;
      }
      prev = lane_d ? Lr : SGM_BIG;
      pm = sgm_group_min<LPS>(prev);
      const unsigned S = ss[k] + (unsigned)Lr;
      if (DIR < 3) {
        if (live) sum[pixel(t) * (size_t)ndisp + i] = S;
        continue;
      }
      // ---- StereoBM's selection on S: the first minimum in i, uniqueness, texture, sub-pixel (S < 2^18)
      const int key = sgm_group_min<LPS>(lane_d ? (int)((S << 6) | (unsigned)i) : SGM_BIG);
      const int minS = key >> 6, mind = key & 63;
      const int thresh = minS + (minS * UNIQUENESS_RATIO / 100);
      const bool rival = lane_d && (i < mind - 1 || i > mind + 1) && (int)S <= thresh;
      const unsigned long long group = (LPS == 64 ? ~0ull : ((1ull << LPS) - 1ull)) << (sub * LPS);
      const bool unique = (__ballot(rival) & group) == 0;
      const int g0 = sub * LPS;
      const int p = __shfl((int)S, g0 + (mind + 1 < ndisp ? mind + 1 : ndisp - 2));
      const int n = __shfl((int)S, g0 + (mind - 1 >= 0 ? mind - 1 : 1));
      if (live && i == 0) {
        int res = SGM_FILTERED, won = 0xFFFF;
        if (tt[k] >= TEXTURE_THRESHOLD && unique) {
          const int dd = p + n - 2 * minS + abs(p - n);
          res = (short)(((ndisp - mind - 1) * 256 + (dd != 0 ? (p - n) * 256 / dd : 0) + 15) >> 4);
          won = min((minS + 2) >> 2, 0xFFFE);
        }
        const int y = a.ry0 + (nsteps - 1 - t), x = a.rx0 + line;
        const size_t o = ((size_t)blockIdx.y * (size_t)a.H + (size_t)y) * (size_t)a.W + (size_t)x;
        a.out[o] = (int16_t)res;
        if (a.cost) a.cost[o] = (uint16_t)won;
      }
    }
  }
}

// ----------------------------------------------------------------------------- host side
namespace {
template <int DIR>
void sgm_launch_path(const SgmArgs& a, int batch, hipStream_t st) {
  const int lps = sgm_lps(a.ndisp);
  const dim3 grid((unsigned)sgm_path_groups(DIR, SgmRect{a.rx0, a.ry0, a.VW, a.VH}, lps), (unsigned)batch);
  if (lps == 16) hipLaunchKernelGGL((sgm_path_kernel<DIR, 16>), grid, dim3(SGM_T), 0, st, a);
  else if (lps == 32) hipLaunchKernelGGL((sgm_path_kernel<DIR, 32>), grid, dim3(SGM_T), 0, st, a);
  else hipLaunchKernelGGL((sgm_path_kernel<DIR, 64>), grid, dim3(SGM_T), 0, st, a);
}
}  // namespace

int svo_k_stereo_sgm(svo_ctx* ctx, const SvoDensePairs& src, int batch, int W, int H, int stride, int ndisp, int block,
                     const svo_sgm_params* prm, void* workspace, int16_t* disp16, uint16_t* cost16) {
  SgmLayout l;
  if (!sgm_layout(W, H, ndisp, block, batch, &l)) { ctx->err = "stereo_sgm: shape outside the limits"; return SVO_ERR_INVALID; }
  const size_t sad_lds = sgm_sad_lds(ndisp);
  if ((int)sad_lds > ctx->sgm_lds_granted) {  // per context (= per device), as the dense kernels' grants
    SVO_HIP_CHECK(ctx, hipFuncSetAttribute((const void*)sgm_volume_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, SGM_LDS_MAX));
    ctx->sgm_lds_granted = SGM_LDS_MAX;
  }
  SgmArgs a{};
  a.src = src; a.W = W; a.H = H; a.stride = stride; a.ndisp = ndisp; a.block = block;
  const SgmRect r = sgm_rect(W, H, ndisp, block);
  a.rx0 = r.rx0; a.ry0 = r.ry0; a.VW = r.VW; a.VH = r.VH;
  a.p1 = prm->p1; a.p2 = prm->p2;
  uint8_t* const ws = static_cast<uint8_t*>(workspace);
  a.vol = reinterpret_cast<uint16_t*>(ws + l.vol);
  a.sum = reinterpret_cast<uint32_t*>(ws + l.sum);
  a.tex = reinterpret_cast<uint16_t*>(ws + l.tex);
  a.out = disp16; a.cost = cost16;
  hipStream_t st = ctx->stream;
  SvoProfScope prof(ctx, SVO_PROF_STEREO_SGM);
  const size_t n = (size_t)batch * (size_t)W * (size_t)H;
  hipLaunchKernelGGL(sgm_fill_kernel, dim3((unsigned)((n + SGM_T - 1) / SGM_T)), dim3(SGM_T), 0, st, disp16, cost16, n);
  if (a.VW > 0 && a.VH > 0) {
    hipLaunchKernelGGL(sgm_volume_kernel, dim3(svo_div_up(a.VW, DT_W), svo_div_up(a.VH, DT_H), batch), dim3(SGM_T), sad_lds, st, a);
    sgm_launch_path<0>(a, batch, st);
    sgm_launch_path<1>(a, batch, st);
    sgm_launch_path<2>(a, batch, st);
    sgm_launch_path<3>(a, batch, st);
  }
  SVO_HIP_CHECK(ctx, hipGetLastError());
  return SVO_OK;
}

extern "C" int svo_sgm_default_params(svo_sgm_params* p, int block_size) { return sgm_default_params(p, block_size); }

extern "C" size_t svo_sgm_workspace_bytes(int width, int height, int num_disparities, int block_size, int batch) {
  return sgm_workspace_bytes(width, height, num_disparities, block_size, batch);
}

extern "C" int svo_stereo_sgm_batch_dev(svo_ctx* ctx, const uint8_t* left, const uint8_t* right, int batch, int width, int height,
                                        int row_stride, size_t image_stride, int num_disparities, int block_size,
                                        const svo_sgm_params* params, void* workspace, size_t workspace_bytes, int16_t* disp16,
                                        uint16_t* cost16) {
  int rc = svo_stereo_check(ctx, left, right, width, height, row_stride, num_disparities, block_size);
  if (rc) return rc;
  SVO_REQUIRE(ctx, disp16, STEREO_SGM_BATCH_TEXTS.null_disp);
  SVO_REQUIRE(ctx, workspace, "stereo_sgm: null workspace");
  SVO_ARGS_CHECK(ctx, dense_batch_check(batch, ctx->lim.max_batch, width, height, row_stride, image_stride, STEREO_SGM_BATCH_TEXTS, &err));
  SVO_ARGS_CHECK(ctx, sgm_check(width, height, num_disparities, block_size, batch, params, &err));
  SVO_REQUIRE(ctx, workspace_bytes >= sgm_workspace_bytes(width, height, num_disparities, block_size, batch),
              "stereo_sgm: workspace_bytes is less than svo_sgm_workspace_bytes for this call");
  SvoDensePairs src{left, right, image_stride, nullptr};
  return svo_k_stereo_sgm(ctx, src, batch, width, height, row_stride, num_disparities, block_size, params, workspace, disp16, cost16);
}

extern "C" int svo_stereo_sgm(svo_ctx* ctx, const uint8_t* left, const uint8_t* right, int width, int height, int row_stride,
                              int num_disparities, int block_size, const svo_sgm_params* params, int16_t* disp16, uint16_t* cost16) {
  int rc = svo_stereo_check(ctx, left, right, width, height, row_stride, num_disparities, block_size);
  if (rc) return rc;
  SVO_REQUIRE(ctx, disp16, STEREO_SGM_BATCH_TEXTS.null_disp);
  SVO_ARGS_CHECK(ctx, sgm_check(width, height, num_disparities, block_size, 1, params, &err));
  // the volume of one pair is far larger than the context's scratch: one allocation for this call, freed before it returns
  const size_t px = (size_t)width * (size_t)height;
  const SgmOneShot o = sgm_one_shot(sgm_workspace_bytes(width, height, num_disparities, block_size, 1), px);
  SvoTemp d;
  SVO_HIP_CHECK(ctx, hipMalloc(&d.p, o.total));
  hipStream_t st = ctx->stream;
  int16_t* dD = d.at<int16_t>(o.disp);
  uint16_t* dC = d.at<uint16_t>(o.cost);
  hipError_t e = hipMemcpy2DAsync(d.at(o.left), width, left, row_stride, width, height, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpy2DAsync(d.at(o.right), width, right, row_stride, width, height, hipMemcpyHostToDevice, st);
  return svo_host_call(
      ctx, "stereo_sgm", e,
      [&] {
        SvoDensePairs src{d.at(o.left), d.at(o.right), px, nullptr};
        return svo_k_stereo_sgm(ctx, src, 1, width, height, width, num_disparities, block_size, params, d.p, dD, cost16 ? dC : nullptr);
      },
      [&] {
        hipError_t e = hipMemcpyAsync(disp16, dD, px * sizeof(int16_t), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && cost16) e = hipMemcpyAsync(cost16, dC, px * sizeof(uint16_t), hipMemcpyDeviceToHost, st);
        return e;
      });
}
