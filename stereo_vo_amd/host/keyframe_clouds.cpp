// The keyframe clouds of one pipeline or one group (csrc/kernels.h, "SvoKfClouds"): the buffers, the three switches and the
// sequence of launches per call.  No kernel lives here: the matchers and the cloud passes are csrc/dense.hip and csrc/sgm.hip, the
// filters csrc/lr_check.hip and csrc/speckle.hip; every rule and every size is host/dense_args.h's.
#include <new>

#include "dense_args.h"
#include "kernels.h"
#include "ref_constants.h"

static_assert(sizeof(SvoCloudPair) == KFC_PAIR_BYTES, "kfc_bytes sizes the pair table");

constexpr int KF_NDISP = svo_ref::STEREO_NUM_DISPARITIES, KF_BLOCK = svo_ref::STEREO_BLOCK_SIZE;

// One optional stage of run(): its parameters while it is on, and the one buffer it needs.
template <typename P>
struct KfcStage {
  bool on = false;
  P prm{};
  void* buf = nullptr;
};

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
  KfcStage<svo_speckle_params> speckle;  // svo_kfc_set_speckle: the maps are filtered before the clouds are formed; buf: speckle_workspace_bytes(W, H, max_kf)
  KfcStage<svo_lr_check_params> lr;      // svo_kfc_set_lr_check: the cost form of the dense launch, then the left-right check; buf: max_kf cost maps
  KfcStage<svo_sgm_params> sgm;          // svo_kfc_set_sgm: semi-global matching (sgm.hip) instead of the dense launch; buf: its workspace for SVO_SGM_KEYFRAME_SUB_BATCH pairs, whatever max_kf is
  std::vector<svo_keyframe_cloud> table;
  uint16_t* d_cost() const { return static_cast<uint16_t*>(lr.buf); }
};

void svo_kfc_destroy(SvoKfClouds* k) {
  if (!k) return;
  (void)hipSetDevice(k->ctx->device);
  (void)hipStreamSynchronize(k->ctx->stream);
  void* ptrs[] = {k->d_disp, k->d_points, k->d_counts, k->d_seg, k->d_tab, k->speckle.buf, k->lr.buf, k->sgm.buf};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  if (k->h_pinned) (void)hipHostFree(k->h_pinned);
  delete k;
}

int svo_kfc_create(svo_ctx* ctx, const svo_cloud_params* params, int W, int H, int max_kf, SvoKfClouds** out) {
  *out = nullptr;
  svo_use_device(ctx);
  svo_cloud_params prm;
  SVO_ARGS_CHECK(ctx, kfc_resolve(params, W, H, max_kf, ctx->lim.max_batch, &prm, &max_kf, &err));
  SvoKfClouds* k = new (std::nothrow) SvoKfClouds();
  if (!k) return SVO_ERR_HIP;
  k->ctx = ctx; k->prm = prm; k->W = W; k->H = H; k->max_kf = max_kf;
  const KfcBytes b = kfc_bytes(W, H, prm, max_kf);
  hipError_t e = hipMalloc((void**)&k->d_disp, b.disp);
  if (e == hipSuccess) e = hipMalloc((void**)&k->d_points, b.points);
  if (e == hipSuccess) e = hipMalloc((void**)&k->d_counts, b.counts);
  if (e == hipSuccess) e = hipMalloc((void**)&k->d_seg, b.seg);
  if (e == hipSuccess) e = hipMalloc((void**)&k->d_tab, b.tab);
  if (e == hipSuccess) e = hipHostMalloc(&k->h_pinned, b.pinned, hipHostMallocDefault);
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

// A stage's switch, after the stage's own check of prm.  prm == null: off, once the stream has drained, and the buffer goes.
// Otherwise the buffer of `bytes` is allocated by the first call that switches the stage on; a failure is reported under
// `alloc_text`, the entry's own.
template <typename P>
static int kfc_switch(SvoKfClouds* k, KfcStage<P>& s, const P* prm, size_t bytes, const char* alloc_text) {
  svo_ctx* ctx = k->ctx;
  svo_use_device(ctx);
  if (!prm) {
    SVO_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    if (s.buf) (void)hipFree(s.buf);
    s.buf = nullptr;
    s.on = false;
    return SVO_OK;
  }
  if (!s.buf) {
    const hipError_t e = hipMalloc(&s.buf, bytes);
    if (e != hipSuccess) {
      s.buf = nullptr;
      ctx->err = std::string(alloc_text) + hipGetErrorString(e);
      return SVO_ERR_HIP;
    }
  }
  s.prm = *prm;
  s.on = true;
  return SVO_OK;
}

int svo_kfc_set_speckle(SvoKfClouds* k, const svo_speckle_params* prm) {
  if (prm) SVO_ARGS_CHECK(k->ctx, speckle_check(k->W, k->H, k->max_kf, prm, &err));
  return kfc_switch(k, k->speckle, prm, speckle_workspace_bytes(k->W, k->H, k->max_kf), "set_keyframe_speckle_filter: allocation failed: ");
}

int svo_kfc_set_lr_check(SvoKfClouds* k, const svo_lr_check_params* prm) {
  if (prm) SVO_ARGS_CHECK(k->ctx, lr_check_check(k->W, k->H, k->max_kf, prm, &err));
  return kfc_switch(k, k->lr, prm, kfc_cost_bytes(k->W, k->H, k->max_kf), "set_keyframe_lr_check: allocation failed: ");
}

int svo_kfc_set_sgm(SvoKfClouds* k, const svo_sgm_params* prm) {
  if (prm) SVO_ARGS_CHECK(k->ctx, sgm_check(k->W, k->H, KF_NDISP, KF_BLOCK, SVO_SGM_KEYFRAME_SUB_BATCH, prm, &err));
  return kfc_switch(k, k->sgm, prm, sgm_workspace_bytes(k->W, k->H, KF_NDISP, KF_BLOCK, SVO_SGM_KEYFRAME_SUB_BATCH),
                    "set_keyframe_sgm: allocation failed: ");
}

int svo_kfc_replace(svo_ctx* ctx, SvoKfClouds** slot, const svo_cloud_params* params, int W, int H, int max_keyframes) {
  SvoKfClouds* k = nullptr;
  int rc = svo_kfc_create(ctx, params, W, H, max_keyframes, &k);
  if (rc) return rc;
  // new buffers for other cloud parameters: a speckle filter, a left-right check and semi-global matching that were on stay on
  const SvoKfClouds* old = *slot;
  if (old && old->speckle.on) rc = svo_kfc_set_speckle(k, &old->speckle.prm);
  if (!rc && old && old->lr.on) rc = svo_kfc_set_lr_check(k, &old->lr.prm);
  if (!rc && old && old->sgm.on) rc = svo_kfc_set_sgm(k, &old->sgm.prm);
  if (rc) { svo_kfc_destroy(k); return rc; }
  svo_kfc_destroy(*slot);
  *slot = k;
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
  SVO_ARGS_CHECK(ctx, cloud_check(k->W, k->H, k->W, cam, &one, ctx->lim.max_width, ctx->lim.max_height, &err));
  int rc = SVO_OK;
  hipStream_t st = ctx->stream;
  SvoCloudPair* h_tab = static_cast<SvoCloudPair*>(k->h_pinned);
  int* h_counts = reinterpret_cast<int*>(h_tab + k->max_kf);
  memcpy(h_tab, pairs, sizeof(SvoCloudPair) * (size_t)n);
  SVO_HIP_CHECK(ctx, hipMemcpyAsync(k->d_tab, h_tab, sizeof(SvoCloudPair) * (size_t)n, hipMemcpyHostToDevice, st));
  SvoDensePairs src{nullptr, nullptr, 0, k->d_tab};
  if (k->sgm.on) {  // the matching sequence per sub-batch: the one workspace is reused, the launches are ordered by the stream
    const size_t px = (size_t)k->W * (size_t)k->H;
    for (int b0 = 0; b0 < n; b0 += SVO_SGM_KEYFRAME_SUB_BATCH) {
      SvoDensePairs sub{nullptr, nullptr, 0, k->d_tab + b0};
      rc = svo_k_stereo_sgm(ctx, sub, kfc_sub_batch(n, b0), k->W, k->H, k->W, KF_NDISP, KF_BLOCK, &k->sgm.prm, k->sgm.buf,
                            k->d_disp + (size_t)b0 * px, k->lr.on ? k->d_cost() + (size_t)b0 * px : nullptr);
      if (rc) return rc;
    }
  } else {
    rc = svo_k_stereo_dense_batch(ctx, src, n, k->W, k->H, k->W, KF_NDISP, KF_BLOCK, k->d_disp, k->lr.on ? k->d_cost() : nullptr);
  }
  if (rc) return rc;
  if (k->lr.on) {  // same stream, before the speckle filter as in StereoBM::compute
    rc = svo_k_lr_check(ctx, k->d_disp, k->d_cost(), n, k->W, k->H, &k->lr.prm, nullptr);
    if (rc) return rc;
  }
  if (k->speckle.on) {  // same stream: the clouds below are those of the filtered maps
    rc = svo_k_speckle(ctx, k->d_disp, n, k->W, k->H, &k->speckle.prm, k->speckle.buf, nullptr);
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
