// Pipeline group: ImageProcessor::process + BundleAdjuster::bundle_adjust (reference src/image_processor.cpp:18-163,
// src/feature_tracker.cpp:18-67, driver rule src/vo_node.cpp:141-148) for SEVERAL stereo streams ("lanes") driven by ONE host
// thread.  Every lane runs the reference's per-frame state machine — exactly the statements of host/pipeline.cpp's
// ImageProcessor::process, cut at the points where the host needs a number from the GPU — and an event loop advances all
// lanes: whatever stage several lanes reach in the same pass goes out as ONE launch (csrc/group_kernels.h, blockIdx.y =
// lane) and the solves of the lanes that hit a keyframe together are one ba_lm_kernel launch.  Lanes never wait for each
// other: a lane whose frame is no keyframe starts tracking its next frame while another lane is still in its PnP.
//
// Why (measured in round 2, profiles/r02_exp_launch_rate.txt, r02_exp_placement.txt, r02_kernel_stats_*): eight streams
// as eight host threads on 16-24 hardware queues pay 30-90 us per launch -> completion round trip (7-11 us with at most
// four queues) and their small kernels run 3-5x their solo time.  Here: one driver thread, four HIP streams (tracking +
// front end, keyframe chain, two for solves), a small pool of host workers that only assemble bundle-adjustment problems.
// Results per lane are bit for bit those of its own svo_pipeline (tests/test_group.py).
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <sched.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <thread>
#include <vector>

#include "chain_math.h"
#include "dense_args.h"
#include "det_trig.h"
#include "group_kernels.h"
#include "group_lines.h"
#include "ref_constants.h"
#include "svo.h"

namespace {

// LM iterations per launch after which a lane's wide window solve steps aside and rides the group's next wide launch (0: never):
// a wide launch holds its solve line, and the hardware queue behind it, as long as its LONGEST solve runs.  SVO_BA_YIELD_ITERS
// overrides, svo_pipeline_group_set_solve_yield sets it for a group.  The default is the best median of profiles/r09_yield_sweep.txt.
constexpr int GROUP_SOLVE_YIELD_DEFAULT = 8;
int group_solve_yield_default() {
  const char* e = getenv("SVO_BA_YIELD_ITERS");
  return e && *e ? std::max(0, atoi(e)) : GROUP_SOLVE_YIELD_DEFAULT;
}

enum LaneState { L_IDLE = 0, L_TRACK_WAIT, L_NEED_SOLVE, L_PNP_WAIT, L_TRI_WAIT, L_DONE };
enum BaState { BA_NONE = 0, BA_ASSEMBLING, BA_READY, BA_INFLIGHT, BA_HOST_SOLVING, BA_HOST_DONE };
enum Word { W_TRACK = 0, W_PNP, W_TRI, W_COUNT };
enum Counter { C_LK = 0, C_PNP, C_TRI, C_COUNT };
// statistics of a batch, in the order svo_pipeline_group_last_stats returns them: launches by kind and the lanes they carried; ST_HOST_US
// holds two times instead (microseconds of the driving thread's loop passes that did something, of the call's main loop)
enum Stat { ST_TRACK = 0, ST_PNP, ST_HOST_US, ST_TRI, ST_SOLVE, ST_FRONT_END, ST_COUNT };

struct Lane {
  int lk_line = 0, chain_line = 0;  // the tracking / keyframe-chain line (stream) its launch in flight went to
  // ---- tracker state (FeatureTracker): feature set double-buffered on the device, mirrored in pinned memory
  float* d_xy[2] = {nullptr, nullptr}; float* d_init[2] = {nullptr, nullptr}; long long* d_ids[2] = {nullptr, nullptr};
  float* d_fwd = nullptr; float* d_par = nullptr; uint8_t* d_keep = nullptr;
  float* h_xy[2] = {nullptr, nullptr}; long long* h_ids[2] = {nullptr, nullptr};  // pinned mirrors of the kept set (double-buffered with the device set)
  float* h_kf_xy = nullptr; long long* h_kf_ids = nullptr;  // pinned: the feature set a keyframe hands to the tracker (src/image_processor.cpp:148-162)
  int* h_n = nullptr; float* h_av = nullptr;
  int cur = 0, n = 0, n_initial = 0;
  bool from_host = false;           // the next track reads its features from h_kf_* (tracker (re)initialised by a keyframe)
  const uint8_t* last_pyr = nullptr;
  const uint8_t* last_l0 = nullptr;  // level 0 of last_pyr: inside it, or (within the batch that produced it) the caller's image read in place
  uint8_t* d_own_pyr = nullptr;      // the lane's private clone of its last image's pyramid, used when a whole batch went by without tracking (see Batch::front_end)
  // ---- PnP
  float4* d_store = nullptr; unsigned store_mask = 0;  // device-resident landmark store of the lane, keyed by feature id (get_world_points, src/bundle_adjuster.cpp:159-163)
  double* d_hyp_pose = nullptr; int* d_hyp_count = nullptr; unsigned long long* d_hyp_mask = nullptr;
  double* d_out = nullptr; int* d_nin = nullptr; int* d_inl = nullptr; float* d_trk_xy = nullptr;
  bool pnp_all = false;  // the lane's next PnP launch computes every hypothesis (the first few did not settle the adaptive cap)
  int* h_best = nullptr; int* h_bad = nullptr; double* h_out = nullptr; int* h_nin = nullptr; int* h_inl = nullptr;
  // ---- dedup / sparse stereo / triangulation
  float* d_disp = nullptr;
  int* h_tri_cnt = nullptr; float* h_tri_xy = nullptr; float* h_tri_xyz = nullptr;
  // ---- hand-over words and arrival counters
  int* words = nullptr;             // pinned, W_COUNT words 64 bytes apart
  int seq[W_COUNT] = {};
  unsigned* d_arrive = nullptr;     // device, C_COUNT counters 64 bytes apart (monotone)
  unsigned arrive_total[C_COUNT] = {0, 0, 0};
  // ---- graph + solve (BundleAdjuster)
  svo_ba* ba = nullptr;
  std::atomic<int> ba_state{BA_NONE};
  svo_ba_summary ba_summary{};
  int ba_rc = 0;
  int ba_launch = 0, ba_line = 0;  // which solve launch of the group carries this lane's solve, on which solve line
  unsigned long long ba_ready_seq = 0;  // when its assembled solve was first seen waiting for a launch (0: none waits); the order of admission
  bool ba_yielded = false;              // the solve that waits has run before: it stepped aside after its LM iterations per launch (it keeps its ba_ready_seq)
  bool has_keyframe = false;
  double solved_pose[7] = {1, 0, 0, 0, 0, 0, 0};
  int last_iterations = 0;
  // ---- ImageProcessor state
  float rvec[3] = {0, 0, 0}, tvec[3] = {0, 0, 0};
  // ---- the frame in flight
  int state = L_IDLE;
  bool queued = false;              // the stage the lane waits for has not been launched yet (its completion word still shows the previous launch)
  int frame = 0;                    // index into the batch
  int pending_from = -1;            // first frame of the batch whose pose waits for the running solve
  bool first_keyframe = false;      // the triangulation in flight is frame 0's (src/image_processor.cpp:30-58)
  SvoChainRec* d_chain = nullptr;   // what the lane's PnP launch leaves for the stereo + triangulation launch queued behind it (host/chain_math.h)
  double t_q = 0.0;                 // when the lane entered the queue of its next stage (microseconds of this call): the gather policy
  bool fused = false;               // the triangulation in flight rides behind a PnP launch: its results are consumed together with PnP's
  int m_tracked = 0, num_inliers = 0, best = -1;
  float rmat[9], quat[4];
  std::vector<long long> kf_tracked_ids; std::vector<float> kf_tracked_xy;  // the keyframe under construction
  std::vector<long long> ids64; std::vector<int64_t> new_ids;
};

struct Pool {  // host workers: they only assemble bundle-adjustment problems (and run the rare host-driven solve)
  std::vector<std::thread> th;
  std::mutex mu;
  std::condition_variable cv;
  std::deque<std::pair<Lane*, int>> jobs;  // (lane, 0: assemble / 1: host-driven solve)
  bool quit = false;
  int device = 0;
  void start(int n, int dev) {
    device = dev;
    for (int i = 0; i < n; ++i) th.emplace_back([this] { run(); });
  }
  void post(Lane* l, int what) {
    { std::lock_guard<std::mutex> g(mu); jobs.emplace_back(l, what); }
    cv.notify_one();
  }
  void run() {
    (void)hipSetDevice(device);
    for (;;) {
      std::pair<Lane*, int> j;
      {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [this] { return quit || !jobs.empty(); });
        if (quit && jobs.empty()) return;
        j = jobs.front(); jobs.pop_front();
      }
      Lane* l = j.first;
      if (j.second == 0) {
        l->ba_rc = svo_ba_solve_prepare(l->ba);
        l->ba_state.store(BA_READY, std::memory_order_release);
      } else {
        l->ba_rc = svo_ba_solve_finish(l->ba, &l->ba_summary);
        l->ba_state.store(BA_HOST_DONE, std::memory_order_release);
      }
    }
  }
  void stop() {
    { std::lock_guard<std::mutex> g(mu); quit = true; }
    cv.notify_all();
    for (auto& t : th) t.join();
    th.clear();
  }
};

}  // namespace

struct svo_pipeline_group {
  svo_ctx* ctx = nullptr;
  svo_pipeline_params prm{};
  int n_lanes = 0, max_batch = 0;
  float K[9];
  std::vector<Lane*> lanes;
  std::vector<void*> dev_allocs, pin_allocs;
  // bus lines: a lane always rides the same tracking line and the same keyframe-chain line (stream order keeps its
  // consecutive stages coherent), solves take whichever solve line is free
  static constexpr int MAX_LINES = 8;
  int n_lk = 1, n_chain = 1, n_ba = 2;
  int n_cmp = 0;  // compact lines: st_ba[n_ba ..): solves the admission budget refuses leave at once in the one-workgroup form, on lines of their own
  int xcd_chunks = SVO_XCD_CHUNKS;
  bool xcd_map = true, xcd_map_tri = true;  // the XCD-aware item -> workgroup map of the tracking / stereo launches (group_kernels.h; SVO_GROUP_LK_XCD=0, SVO_GROUP_TRI_XCD=0: blockIdx = (item, lane))
  // SVO_TIMING: host time of the group thread inside the per-keyframe graph calls (ns), and keyframes seen
  double t_get_points = 0, t_add_keyframe = 0, t_finish = 0, t_loop = 0; long n_kf = 0; bool timing = false;
  double gather_us = 0.0;      // > 0: a stage's launch waits up to this long for the other lanes of its line that are still on their way
  hipStream_t st_lk[MAX_LINES] = {}, st_chain[MAX_LINES] = {}, st_ba[MAX_LINES] = {};
  int ba_launch_id = 0;
  unsigned long long ba_ready_counter = 0;
  // batch-wide front-end outputs
  float* d_corners = nullptr; int* d_ncorners = nullptr; uint8_t* d_pyr[2] = {nullptr, nullptr}; int pyr_cur = 0;
  size_t pyr_stride = 0;
  int* h_counts = nullptr;  // pinned: n_lanes x max_batch corner counts + status
  Pool pool;
  int pnp_iterations = 0, mask_words_cap = 0;
  long launches[ST_COUNT] = {}, lanes_carried[ST_COUNT] = {};  // statistics of the last batch (enum Stat)
  // host-pointer / streaming entry: two pinned staging slots, their device twins, a copy stream (allocated on first use)
  uint8_t* h_stage[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};  // [slot][left / right]
  uint8_t* d_stage[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
  hipStream_t st_copy = nullptr;
  hipEvent_t ev_up[2] = {nullptr, nullptr};
  int up_batch[2] = {0, 0};  // frames per lane of the upload in flight / completed in the slot (0: none)
  // raw input (svo_pipeline_group_set_rectification): the distinct cameras' tables, which one each lane uses (null: the lane's
  // images are rectified already), and the rectified workspace [left / right]: n_lanes x max_batch images, allocated with the first model
  std::vector<SvoRectModel*> rect_models;
  SvoRectModel* lane_rect[SVO_MAX_LANES] = {};
  uint8_t* d_rect[2] = {nullptr, nullptr};
  // keyframe clouds (svo_pipeline_group_set_keyframe_clouds): one set of buffers for the lanes that have them on (null: none has)
  SvoKfClouds* kfc = nullptr;
  bool lane_cloud[SVO_MAX_LANES] = {};
};

namespace {

int fail(svo_pipeline_group* g, const char* what, hipError_t e) {
  g->ctx->err = std::string("pipeline group: ") + what + ": " + hipGetErrorString(e);
  return SVO_ERR_HIP;
}

template <typename T>
int dev_alloc(svo_pipeline_group* g, T** p, size_t count) {
  const hipError_t e = hipMalloc((void**)p, sizeof(T) * (count ? count : 1));
  if (e != hipSuccess) return fail(g, "hipMalloc", e);
  g->dev_allocs.push_back(*p);
  return SVO_OK;
}

int word_ready(const Lane* l, int w) { return __atomic_load_n(&l->words[16 * w], __ATOMIC_ACQUIRE) == l->seq[w]; }

SvoPublish make_pub(Lane* l, int w, int counter, int nblocks) {
  SvoPublish p;
  p.word = &l->words[16 * w];
  p.seq = ++l->seq[w];
  if (counter >= 0) {
    l->arrive_total[counter] += (unsigned)nblocks;
    p.arrive = l->d_arrive + 16 * counter;
    p.target = l->arrive_total[counter];
  }
  return p;
}

void fill_pending(Lane* l, svo_frame_result* res, int upto) {
  if (l->pending_from < 0) return;
  for (int j = l->pending_from; j < upto; ++j) {
    memcpy(res[j].pose7, l->solved_pose, sizeof(res[j].pose7));
    if (j == l->pending_from && res[j].is_keyframe) res[j].ba_iterations = l->last_iterations;
  }
  l->pending_from = -1;
}

// join the lane's solve (BundleAdjuster::bundle_adjust's tail, src/bundle_adjuster.cpp:146-155; host/pipeline.cpp run_bundle_adjust)
int finish_solve(svo_pipeline_group* g, Lane* l) {
  const int st = l->ba_state.load(std::memory_order_acquire);
  l->ba_ready_seq = 0;  // (no solve of this lane waits for a launch any more)
  l->ba_yielded = false;
  if (st == BA_NONE) return SVO_OK;
  int rc = SVO_OK;
  const auto tf0 = std::chrono::steady_clock::now();
  if (st == BA_INFLIGHT) rc = svo_ba_solve_finish(l->ba, &l->ba_summary);
  else rc = l->ba_rc;  // BA_HOST_DONE
  if (g->timing) g->t_finish += std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - tf0).count();
  l->ba_state.store(BA_NONE, std::memory_order_release);
  if (rc) return rc;
  l->last_iterations = l->ba_summary.iterations;
  double p[7];
  if ((rc = svo_ba_get_pose(l->ba, -1, p))) return rc;
  for (int i = 0; i < 7; ++i) l->solved_pose[i] = (double)(float)p[i];  // Keyframe holds Quaternionf / Vector3f (:146-153)
  (void)g;
  return SVO_OK;
}

// After a failed batch: launches of other lanes may still be in flight (they read the caller's images and write the pinned
// mirrors and completion words), and arrive_total[] / seq[] were advanced for launches that may never have run.  Drain every
// line, then bring device counters, host totals and completion words back to a common zero.
void quiesce_after_error(svo_pipeline_group* g) {
  for (int i = 0; i < svo_pipeline_group::MAX_LINES; ++i) {
    if (g->st_lk[i]) (void)hipStreamSynchronize(g->st_lk[i]);
    if (g->st_chain[i]) (void)hipStreamSynchronize(g->st_chain[i]);
    if (g->st_ba[i]) (void)hipStreamSynchronize(g->st_ba[i]);
  }
  for (Lane* l : g->lanes) {
    (void)hipMemset(l->d_arrive, 0, sizeof(unsigned) * 16 * C_COUNT);
    for (int c = 0; c < C_COUNT; ++c) l->arrive_total[c] = 0;
    for (int w = 0; w < W_COUNT; ++w) { l->seq[w] = 0; l->words[16 * w] = 0; }
    if (l->h_bad) *l->h_bad = 0;  // a "foreign landmark-store entry" report must not outlive the batch it failed
    l->fused = false; l->pnp_all = false;
    l->queued = false;
  }
  (void)hipDeviceSynchronize();  // (the fills ran on the null stream)
}

}  // namespace

extern "C" void svo_pipeline_group_destroy(svo_pipeline_group* g) {
  if (!g) return;
  (void)hipSetDevice(g->ctx->device);
  g->pool.stop();
  for (Lane* l : g->lanes) {
    if (l->ba_state.load() == BA_INFLIGHT) { svo_ba_summary s; (void)svo_ba_solve_finish(l->ba, &s); }
  }
  if (g->timing && g->n_kf)
    fprintf(stderr, "[svo group] %d lanes, %ld keyframes; group thread per keyframe (us): get_world_points %.1f, add_keyframe %.1f, join + write-back of the solve %.1f\n",
            g->n_lanes, g->n_kf, 1e-3 * g->t_get_points / g->n_kf, 1e-3 * g->t_add_keyframe / g->n_kf, 1e-3 * g->t_finish / g->n_kf);
  (void)hipStreamSynchronize(g->ctx->stream);
  for (Lane* l : g->lanes) { if (l->ba) { svo_ba_destroy(l->ba); l->ba = nullptr; } }  // before the lines they work on (svo_ba_use_stream) go
  for (int i = 0; i < svo_pipeline_group::MAX_LINES; ++i) {
    if (g->st_lk[i] && g->st_lk[i] != g->ctx->stream) { (void)hipStreamSynchronize(g->st_lk[i]); (void)hipStreamDestroy(g->st_lk[i]); }
    if (g->st_chain[i]) { (void)hipStreamSynchronize(g->st_chain[i]); (void)hipStreamDestroy(g->st_chain[i]); }
    if (g->st_ba[i]) { (void)hipStreamSynchronize(g->st_ba[i]); (void)hipStreamDestroy(g->st_ba[i]); }
  }
  if (g->st_copy) { (void)hipStreamSynchronize(g->st_copy); (void)hipStreamDestroy(g->st_copy); }
  for (int sl = 0; sl < 2; ++sl) {
    if (g->ev_up[sl]) (void)hipEventDestroy(g->ev_up[sl]);
    for (int e = 0; e < 2; ++e) { if (g->h_stage[sl][e]) (void)hipHostFree(g->h_stage[sl][e]); if (g->d_stage[sl][e]) (void)hipFree(g->d_stage[sl][e]); }
  }
  for (Lane* l : g->lanes) { if (l->ba) svo_ba_destroy(l->ba); delete l; }
  svo_kfc_destroy(g->kfc);
  for (SvoRectModel* m : g->rect_models) svo_rect_model_destroy(m);
  for (int e = 0; e < 2; ++e) if (g->d_rect[e]) (void)hipFree(g->d_rect[e]);
  for (void* p : g->dev_allocs) (void)hipFree(p);
  for (void* p : g->pin_allocs) (void)hipHostFree(p);
  delete g;
}

extern "C" int svo_pipeline_group_create(svo_ctx* ctx, svo_pipeline_group** out, const svo_pipeline_params* p, int n_lanes) {
  if (!ctx || !out || !p) return SVO_ERR_INVALID;
  *out = nullptr;
  SVO_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  SVO_REQUIRE(ctx, n_lanes >= 1 && n_lanes <= SVO_MAX_LANES, "pipeline_group_create: 1..64 lanes");
  SVO_REQUIRE(ctx, p->width >= 32 && p->height >= 32 && p->width <= ctx->lim.max_width && p->height <= ctx->lim.max_height,
              "pipeline_group_create: image size outside the context limits");
  SVO_REQUIRE(ctx, p->max_corners >= 4 && p->max_corners <= ctx->lim.max_corners && p->max_features >= 4 &&
                       p->max_features <= ctx->lim.max_features, "pipeline_group_create: feature counts outside the context limits");
  SVO_REQUIRE(ctx, p->window_size >= 1 && p->window_size <= 63, "pipeline_group_create: window size must be 1..63");
  SVO_REQUIRE(ctx, ctx->lim.max_batch >= n_lanes, "pipeline_group_create: svo_limits.max_batch must hold lanes x frames per call");
  {
    // A group drives 1 + chain + solve lines (HIP streams); the runtime maps streams onto GPU_MAX_HW_QUEUES hardware queues
    // (default 4, read when the runtime initialises).  With fewer queues than lines a 1 ms solve launch shares a queue with
    // tracking launches and serialises them: measured 9.9 k against 16+ k frames/s for 48 lanes.
    static std::atomic<bool> warned{false};
    const char* q = getenv("GPU_MAX_HW_QUEUES");
    const int nq = q && *q ? atoi(q) : 4;
    if (n_lanes > 4 && nq < 8 && !warned.exchange(true))
      fprintf(stderr, "[svo] pipeline group of %d lanes with GPU_MAX_HW_QUEUES=%d: its launches will share hardware queues and serialise; "
                      "export GPU_MAX_HW_QUEUES=16 before the first HIP call (INTEGRATION.md)\n", n_lanes, nq);
  }
  svo_pipeline_group* g = new svo_pipeline_group();
  g->ctx = ctx; g->prm = *p; g->n_lanes = n_lanes;
  g->max_batch = ctx->lim.max_batch / n_lanes;
  const float K[9] = {(float)p->cam.focal, 0.f, (float)p->cam.cx, 0.f, (float)p->cam.focal, (float)p->cam.cy, 0.f, 0.f, 1.f};  // src/vo_node.cpp:104-108
  memcpy(g->K, K, sizeof(K));
  g->pnp_iterations = svo_ref::PNP_ITERATIONS;
  const size_t mc = (size_t)p->max_corners, mf = (size_t)ctx->lim.max_features, B = (size_t)g->max_batch, S = (size_t)n_lanes;
  const int words = (int)((mf + 63) / 64);
  g->mask_words_cap = words;
  int rc = SVO_OK;
  auto chk = [&](hipError_t e, const char* what) { if (rc == SVO_OK && e != hipSuccess) rc = fail(g, what, e); };
  {
    auto knob = [](const char* name, int dflt, int hi) { const char* e = getenv(name); int v = e && *e ? atoi(e) : dflt; return v < 1 ? 1 : (v > hi ? hi : v); };
    g->n_lk = knob("SVO_GROUP_LK_LINES", 1, svo_pipeline_group::MAX_LINES);
    g->timing = getenv("SVO_TIMING") != nullptr;
    { const char* e = getenv("SVO_GROUP_GATHER_US"); g->gather_us = e && *e ? std::max(0.0, atof(e)) : 0.0; }
    g->n_chain = knob("SVO_GROUP_CHAIN_LINES", 2, svo_pipeline_group::MAX_LINES);
    { const char* e = getenv("SVO_GROUP_LK_XCD"); g->xcd_map = !(e && *e && atoi(e) == 0); }
    { const char* e = getenv("SVO_GROUP_TRI_XCD"); g->xcd_map_tri = !(e && *e && atoi(e) == 0); }
    { const char* e = getenv("SVO_GROUP_XCD_CHUNKS"); if (e && *e) g->xcd_chunks = std::max(8, std::min(64, atoi(e) / 8 * 8)); }  // developer experiments
    g->n_ba = knob("SVO_GROUP_BA_LINES", 4, svo_pipeline_group::MAX_LINES);
    { const char* e = getenv("SVO_GROUP_COMPACT_LINES"); g->n_cmp = e && *e ? std::max(0, std::min(atoi(e), svo_pipeline_group::MAX_LINES - g->n_ba)) : 0; }
    // plain streams for every line: high-priority chain lines, solve lines of another priority class, the tracker on fewer CUs
    // were all measured slower (profiles/r03_group_sweep.txt, r05_exp_lanes_groups*.txt)
    g->st_lk[0] = ctx->stream;
    for (int i = 1; i < g->n_lk; ++i) chk(hipStreamCreateWithFlags(&g->st_lk[i], hipStreamNonBlocking), "stream");
    for (int i = 0; i < g->n_chain; ++i) chk(hipStreamCreateWithFlags(&g->st_chain[i], hipStreamNonBlocking), "stream");
    for (int i = 0; i < g->n_ba + g->n_cmp; ++i) chk(hipStreamCreateWithFlags(&g->st_ba[i], hipStreamNonBlocking), "stream");
  }
  g->pyr_stride = svo_k_pyramid_bytes(p->width, p->height);
  if (!rc) rc = dev_alloc(g, &g->d_corners, 2 * mc * S * B);
  if (!rc) {
    // The runtime binds a HIP stream to one of its GPU_MAX_HW_QUEUES hardware queues when the stream is first USED (the least
    // referenced queue at that moment); streams that share a hardware queue serialise.  With several groups warming up on their
    // own threads the order of first use — and with it which streams end up sharing a queue — differed from run to run (the same
    // command gave 22 k or 41 k frames/s at 128 lanes in 4 groups, profiles/r05_exp_lanes_groups.txt).  Touch every line once, here,
    // on the creating thread, in a fixed order: the binding becomes a function of the creation order alone.  SVO_GROUP_TOUCH=0: off.
    const char* e = getenv("SVO_GROUP_TOUCH");
    if (!(e && *e && atoi(e) == 0)) {
      hipStream_t order[3 * svo_pipeline_group::MAX_LINES];
      int no = 0;
      for (int i = 0; i < g->n_ba + g->n_cmp; ++i) order[no++] = g->st_ba[i];
      for (int i = 0; i < g->n_chain; ++i) order[no++] = g->st_chain[i];
      for (int i = 0; i < g->n_lk; ++i) order[no++] = g->st_lk[i];
      for (int i = 0; i < no && !rc; ++i) {
        chk(hipMemsetAsync(g->d_corners, 0, 16, order[i]), "hipMemsetAsync");
        chk(hipStreamSynchronize(order[i]), "hipStreamSynchronize");
      }
    }
  }
  if (!rc) rc = dev_alloc(g, &g->d_ncorners, S * B);
  if (!rc) rc = dev_alloc(g, &g->d_pyr[0], g->pyr_stride * S * B);
  if (!rc) rc = dev_alloc(g, &g->d_pyr[1], g->pyr_stride * S * B);
  if (!rc) {
    void* hp = nullptr;
    chk(hipHostMalloc(&hp, sizeof(int) * (S * B + 16), hipHostMallocDefault), "hipHostMalloc");
    if (hp) { g->pin_allocs.push_back(hp); g->h_counts = (int*)hp; memset(hp, 0, sizeof(int) * (S * B + 16)); }
  }
  for (int li = 0; li < n_lanes && !rc; ++li) {
    Lane* l = new Lane();
    g->lanes.push_back(l);
    for (int b = 0; b < 2 && !rc; ++b) {
      rc = dev_alloc(g, &l->d_xy[b], 2 * mf);
      if (!rc) rc = dev_alloc(g, &l->d_init[b], 2 * mf);
      if (!rc) rc = dev_alloc(g, &l->d_ids[b], mf);
    }
    if (!rc) rc = dev_alloc(g, &l->d_fwd, 2 * mf);
    if (!rc) rc = dev_alloc(g, &l->d_par, mf);
    if (!rc) rc = dev_alloc(g, &l->d_keep, mf);
    {
      // ids advance by at most max_features per keyframe: room for 256 keyframes of survival, power of two; an entry found
      // under another id is reported by the PnP launch (never used silently)
      size_t cap = 1, keyframes = 256;
      if (const char* e = getenv("SVO_GROUP_STORE_KEYFRAMES")) keyframes = (size_t)std::max(1, atoi(e));  // test hook: a store too small must fail loudly (tests/test_group.py)
      while (cap < keyframes * mf) cap <<= 1;
      l->store_mask = (unsigned)(cap - 1);
      if (!rc) rc = dev_alloc(g, &l->d_store, cap);
      if (!rc) chk(hipMemset(l->d_store, 0xFF, sizeof(float4) * cap), "hipMemset");
    }
    if (!rc) rc = dev_alloc(g, &l->d_hyp_pose, 7 * (size_t)g->pnp_iterations);
    if (!rc) rc = dev_alloc(g, &l->d_hyp_count, (size_t)g->pnp_iterations);
    if (!rc) rc = dev_alloc(g, &l->d_hyp_mask, (size_t)g->pnp_iterations * words);
    if (!rc) rc = dev_alloc(g, &l->d_out, 8);
    if (!rc) rc = dev_alloc(g, &l->d_nin, 16);
    if (!rc) rc = dev_alloc(g, &l->d_inl, mf);
    if (!rc) rc = dev_alloc(g, &l->d_trk_xy, 2 * mf);
    if (!rc) rc = dev_alloc(g, &l->d_chain, 1);
    if (!rc) rc = dev_alloc(g, &l->d_disp, mc);
    if (!rc) rc = dev_alloc(g, &l->d_own_pyr, g->pyr_stride);
    if (!rc) rc = dev_alloc(g, &l->d_arrive, 16 * C_COUNT);
    if (!rc) chk(hipMemset(l->d_arrive, 0, sizeof(unsigned) * 16 * C_COUNT), "hipMemset");
    if (rc) break;
    // one pinned arena per lane
    const size_t f2 = sizeof(float) * 2 * mf, i8 = sizeof(long long) * mf;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off = (off + bytes + 127) & ~(size_t)127; return o; };
    const size_t o_xy0 = take(f2), o_xy1 = take(f2), o_id0 = take(i8), o_id1 = take(i8), o_kxy = take(f2), o_kid = take(i8), o_n = take(64),
                 o_cnt = take(64), o_out = take(64), o_nin = take(64),
                 o_inl = take(sizeof(int) * mf), o_tc = take(64), o_txy = take(sizeof(float) * 2 * mc), o_txyz = take(sizeof(float) * 3 * mc),
                 o_words = take(64 * W_COUNT);
    void* hp = nullptr;
    chk(hipHostMalloc(&hp, off, hipHostMallocDefault), "hipHostMalloc");
    if (rc) break;
    g->pin_allocs.push_back(hp);
    memset(hp, 0, off);  // completion words are compared by equality with a sequence number: never start from recycled bytes
    char* h = (char*)hp;
    l->h_xy[0] = (float*)(h + o_xy0); l->h_xy[1] = (float*)(h + o_xy1); l->h_ids[0] = (long long*)(h + o_id0); l->h_ids[1] = (long long*)(h + o_id1);
    l->h_kf_xy = (float*)(h + o_kxy); l->h_kf_ids = (long long*)(h + o_kid);
    l->h_n = (int*)(h + o_n); l->h_av = (float*)(h + o_n + 16);
    l->h_best = (int*)(h + o_cnt); l->h_bad = (int*)(h + o_cnt) + 1; l->h_out = (double*)(h + o_out); l->h_nin = (int*)(h + o_nin);
    l->h_inl = (int*)(h + o_inl); l->h_tri_cnt = (int*)(h + o_tc); l->h_tri_xy = (float*)(h + o_txy); l->h_tri_xyz = (float*)(h + o_txyz);
    l->words = (int*)(h + o_words);
    svo_ba_options opt;
    svo_ba_default_options(&opt);
    opt.max_features = p->max_features;       // src/bundle_adjuster.hpp:75
    opt.max_iterations = p->ba_max_iterations;
    opt.max_time_s = p->ba_max_time_s;        // src/bundle_adjuster.cpp:11
    const int max_obs = (p->window_size + 1) * p->max_features + 64;
    rc = svo_ba_create(ctx, &l->ba, p->window_size, &p->cam, &opt, max_obs, max_obs);
    if (!rc) rc = svo_ba_attach_store(l->ba, l->d_store, l->store_mask);
    // the lane's adjuster works on the group's solve lines (no stream of its own: see the hardware-queue note above)
    if (!rc) rc = svo_ba_use_stream(l->ba, g->st_ba[li % g->n_ba]);
    if (!rc) rc = svo_ba_set_yield_iterations(l->ba, group_solve_yield_default());
    // (the window solves keep the wide form unless SVO_BA_FORM=compact: measured in round 5, one workgroup per solve costs a lane
    // ~10x the solve latency and halves the frame rate at 48 lanes — profiles/r05_exp_compact_lanes.txt; the compact form serves as
    // the overflow of the admission budget, SVO_BA_OVERFLOW, and as the re-run of a solve that gave up)
  }
  if (rc) { svo_pipeline_group_destroy(g); return rc; }
  {
    const char* e = getenv("SVO_GROUP_WORKERS");
    // one worker per lane up to 8: lanes in phase reach their keyframes together, and a problem that waits for a worker
    // delays its solve — measured with 2 workers for 8 lanes: 400 us from add_keyframe to the solve's launch, 90 of them assembly
    int nw = e ? atoi(e) : (n_lanes < 8 ? n_lanes : 8);
    if (nw < 1) nw = 1;
    if (nw > 8) nw = 8;
    g->pool.start(nw, ctx->device);
  }
  (void)hipDeviceSynchronize();  // the fills above ran on the null stream, the group's lines are non-blocking streams: nothing may still be in flight
  *out = g;
  return SVO_OK;
}

extern "C" int svo_pipeline_group_reset(svo_pipeline_group* g) {
  if (!g) return SVO_ERR_INVALID;
  (void)hipSetDevice(g->ctx->device);
  int rc_join = SVO_OK;
  for (Lane* l : g->lanes) {
    const int rcf = finish_solve(g, l);
    if (rcf && !rc_join) rc_join = rcf;
    svo_ba_reset(l->ba);
    l->has_keyframe = false; l->n = l->n_initial = 0; l->from_host = false; l->last_pyr = nullptr; l->last_l0 = nullptr; l->cur = 0;
    l->rvec[0] = l->rvec[1] = l->rvec[2] = l->tvec[0] = l->tvec[1] = l->tvec[2] = 0.f;
    l->state = L_IDLE; l->queued = false; l->pending_from = -1; l->last_iterations = 0;
    const double id7[7] = {1, 0, 0, 0, 0, 0, 0};
    memcpy(l->solved_pose, id7, sizeof(id7));
    // feature ids restart at 0 (svo_ba_reset): no entry of the landmark store may survive under an old id, and a reported
    // foreign entry is forgotten with the stream that produced it
    if (l->h_bad) *l->h_bad = 0;
    l->fused = false; l->pnp_all = false;
    // (on the context's stream and waited for below: hipMemset on device memory may return before the fill has run, and the group's
    // lines are non-blocking streams — a fill that landed behind the first solve of the next batch wiped its entries; seen under rocprofv3)
    if (l->d_store && hipMemsetAsync(l->d_store, 0xFF, sizeof(float4) * ((size_t)l->store_mask + 1), g->ctx->stream) != hipSuccess && !rc_join) rc_join = SVO_ERR_HIP;
  }
  if (hipStreamSynchronize(g->ctx->stream) != hipSuccess && !rc_join) rc_join = SVO_ERR_HIP;
  if (rc_join) { quiesce_after_error(g); return rc_join; }  // a solve that was in flight did not come back cleanly
  return SVO_OK;
}

extern "C" int svo_pipeline_group_lanes(const svo_pipeline_group* g) { return g ? g->n_lanes : 0; }

extern "C" int svo_pipeline_group_get_tracked(svo_pipeline_group* g, int lane, int64_t* ids, float* xy, int capacity, int* n) {
  if (!g || !n || lane < 0 || lane >= g->n_lanes) return SVO_ERR_INVALID;
  const Lane* l = g->lanes[lane];
  *n = l->n;
  const float* sx = l->from_host ? l->h_kf_xy : l->h_xy[l->cur];
  const long long* si = l->from_host ? l->h_kf_ids : l->h_ids[l->cur];
  for (int i = 0; i < l->n && i < capacity; ++i) {
    if (ids) ids[i] = (int64_t)si[i];
    if (xy) { xy[2 * i] = sx[2 * i]; xy[2 * i + 1] = sx[2 * i + 1]; }
  }
  return SVO_OK;
}

extern "C" int svo_pipeline_group_set_solve_yield(svo_pipeline_group* g, int n) {
  if (!g || n < 0) return SVO_ERR_INVALID;
  for (Lane* l : g->lanes) {
    const int rc = svo_ba_set_yield_iterations(l->ba, n);
    if (rc) return rc;
  }
  return SVO_OK;
}

extern "C" int svo_pipeline_group_solve_work(svo_pipeline_group* g, double* out4, int reset) {
  if (!g || !out4) return SVO_ERR_INVALID;
  out4[0] = out4[1] = out4[2] = out4[3] = 0.0;
  for (Lane* l : g->lanes) {
    double w[4];
    svo_ba_work(l->ba, w, reset);
    for (int i = 0; i < 4; ++i) out4[i] += w[i];
  }
  return SVO_OK;
}

extern "C" int svo_pipeline_group_solve_forms(svo_pipeline_group* g, long* counts, int n, long* gave_up) {
  if (!g || !counts || n < 1) return SVO_ERR_INVALID;
  std::vector<long> c((size_t)n);
  for (int i = 0; i < n; ++i) counts[i] = 0;
  if (gave_up) *gave_up = 0;
  for (Lane* l : g->lanes) {
    long gu = 0;
    const int rc = svo_ba_solve_forms(l->ba, c.data(), n, &gu);
    if (rc) return rc;
    for (int i = 0; i < n; ++i) counts[i] += c[(size_t)i];
    if (gave_up) *gave_up += gu;
  }
  return SVO_OK;
}

extern "C" int svo_pipeline_group_last_stats(const svo_pipeline_group* g, long* launches6, long* lanes6) {
  if (!g || !launches6 || !lanes6) return SVO_ERR_INVALID;
  static_assert(ST_COUNT == 6, "svo_pipeline_group_last_stats returns six slots");
  for (int i = 0; i < ST_COUNT; ++i) { launches6[i] = g->launches[i]; lanes6[i] = g->lanes_carried[i]; }
  return SVO_OK;
}

namespace {
bool trace_enabled() { static const bool on = getenv("SVO_GROUP_TRACE") != nullptr; return on; }  // SVO_GROUP_TRACE=1: (microseconds, lane, event) of every call on stderr — where a lane's time goes
// the keyframe chain without a host turn between PnP and stereo + triangulation (round 5); SVO_GROUP_CHAIN_FUSED=0: one launch,
// one host turn each, as before — same results either way (tests/test_group.py)
bool chain_fused_enabled() { static const bool on = [] { const char* e = getenv("SVO_GROUP_CHAIN_FUSED"); return !(e && *e && atoi(e) == 0); }(); return on; }
// test hook: every window down the host-driven path (the landmark store is then filled by the scatter launch)
bool host_solves_only() { static const bool on = [] { const char* e = getenv("SVO_GROUP_HOST_SOLVES"); return e && *e && atoi(e) != 0; }(); return on; }

// One call of the batch entry: what its stages share, the per-lane state machine (start_frame ... frame_done, the statements
// of host/pipeline.cpp's ImageProcessor::process), the launches of a pass and the driver (run).
// lbase[l] / rbase[l]: lane l's `batch` rectified images (tight rows, width*height bytes apart), wherever they live: the
// caller's buffers, or the rectified workspace for a lane with a camera model.
struct Batch {
  using Clock = std::chrono::steady_clock;
  struct Ev { double us; int lane; const char* what; int arg; };
  static constexpr int MAX_LINES = svo_pipeline_group::MAX_LINES;

  svo_pipeline_group* const g;
  svo_ctx* const ctx;
  const uint8_t* const* const lbase;
  const uint8_t* const* const rbase;
  const int batch;
  svo_frame_result* const results;
  const int W, H, S;
  const size_t istride;
  uint8_t* pyr = nullptr;  // this batch's pyramids
  int* hc = nullptr;       // pinned: corner counts of every (lane, frame) + the status word
  std::vector<int> q_track, q_pnp, q_tri, q_ba;  // per-pass submission lists
  int error = SVO_OK;
  const int MODEL = svo_pnp_model_points();
  const bool trace_on = trace_enabled(), chain_fused = chain_fused_enabled();
  std::vector<Ev> evs;
  Clock::time_point t_begin, t_pass, last_progress;
  // ---- the pass in hand
  bool all_done = false, progressed = false;
  bool lk_busy[MAX_LINES] = {}, chain_busy[MAX_LINES] = {}, ba_line_busy[MAX_LINES] = {};  // a launch of the line is in flight
  double t_now_us = 0.0;
  unsigned idle_spins = 0;
  double busy_us = 0.0;  // wall time of the loop passes that did something: how much of the call the driving thread was occupied

  Batch(svo_pipeline_group* g_, const uint8_t* const* lb, const uint8_t* const* rb, int batch_, svo_frame_result* res)
      : g(g_), ctx(g_->ctx), lbase(lb), rbase(rb), batch(batch_), results(res), W(g_->prm.width), H(g_->prm.height), S(g_->n_lanes),
        istride((size_t)g_->prm.width * g_->prm.height) {}

  svo_frame_result& RES(int lane, int f) const { return results[(size_t)lane * batch + f]; }
  const uint8_t* IMG(const uint8_t* const* base, int lane, int f) const { return base[lane] + (size_t)f * istride; }
  uint8_t* PYR(int lane, int f) const { return pyr + ((size_t)lane * batch + f) * g->pyr_stride; }
  // level 0 of frame f's pyramid: the caller's image, except the batch's last frame (copied into the pyramid by front_end)
  const uint8_t* L0(int lane, int f) const { return f == batch - 1 ? PYR(lane, f) : IMG(lbase, lane, f); }
  float* DET(int lane, int f) const { return g->d_corners + ((size_t)lane * batch + f) * 2 * g->prm.max_corners; }
  double now_us() const { return std::chrono::duration<double, std::micro>(Clock::now() - t_begin).count(); }
  void EV(int lane, const char* what, int arg) { if (trace_on) evs.push_back({now_us(), lane, what, arg}); }
  void enqueue(std::vector<int>& q, int li, int state) {  // the lane waits for the next launch of a stage
    Lane* l = g->lanes[li];
    q.push_back(li); l->queued = true; l->t_q = now_us(); l->state = state;
  }
  void count(Stat s, int lanes) { g->launches[s]++; g->lanes_carried[s] += lanes; progressed = true; }

  // ================================================================ the per-lane state machine
  // frame finished (is_keyframe etc. already in the result): move on
  void frame_done(int li) {
    Lane* l = g->lanes[li];
    svo_frame_result* res = &RES(li, 0);
    const int i = l->frame;
    if (l->has_keyframe && !(res[i].is_keyframe) && l->pending_from < 0) l->pending_from = i;  // no solve started here: the pose is the last solved one (src/vo_node.cpp:146-150)
    l->frame = i + 1;
    l->state = l->frame < batch ? L_IDLE : L_DONE;
  }

  // src/image_processor.cpp:137-162 once the triangulated new features are on the host: keyframe, solve, tracker
  int keyframe_tail(int li) {
    Lane* l = g->lanes[li];
    svo_frame_result* res = &RES(li, 0);
    const int i = l->frame;
    const int m_new = *l->h_tri_cnt;
    double pose7[7];
    if (l->first_keyframe) {
      const double id7[7] = {1, 0, 0, 0, 0, 0, 0};  // :41 Vector3f zero, Quaternionf identity
      memcpy(pose7, id7, sizeof(id7));
      l->kf_tracked_ids.clear(); l->kf_tracked_xy.clear();
    } else {
      pose7[0] = l->quat[0]; pose7[1] = l->quat[1]; pose7[2] = l->quat[2]; pose7[3] = l->quat[3];
      pose7[4] = l->tvec[0]; pose7[5] = l->tvec[1]; pose7[6] = l->tvec[2];
    }
    const int nt = (int)l->kf_tracked_ids.size();
    l->new_ids.assign((size_t)(m_new > 0 ? m_new : 1), 0);
    int kept = 0;
    std::vector<int64_t> tid(l->kf_tracked_ids.begin(), l->kf_tracked_ids.end());
    const auto ta0 = Clock::now();
    int rc2 = svo_ba_add_keyframe(l->ba, pose7, tid.data(), l->kf_tracked_xy.data(), nt, l->h_tri_xy, l->h_tri_xyz, m_new, l->new_ids.data(), &kept);  // :144
    if (g->timing) { g->t_add_keyframe += std::chrono::duration<double, std::nano>(Clock::now() - ta0).count(); g->n_kf++; }
    if (rc2) return rc2;
    // the previous solve was joined before the graph was edited: its poses are final now
    fill_pending(l, res, i);
    l->pending_from = i;
    l->has_keyframe = true;
    l->ba_state.store(BA_ASSEMBLING, std::memory_order_release);  // src/vo_node.cpp:147, started here so that the assembly overlaps the next frames
    g->pool.post(l, 0);
    EV(li, "assembly_posted", i);
    // tracker->init(left, tracked + new, ids) :148-162 — the next track reads these pinned arrays in place
    int n = nt + kept;
    if (n > ctx->lim.max_features) n = ctx->lim.max_features;
    for (int k = 0; k < nt && k < n; ++k) { l->h_kf_xy[2 * k] = l->kf_tracked_xy[2 * k]; l->h_kf_xy[2 * k + 1] = l->kf_tracked_xy[2 * k + 1]; l->h_kf_ids[k] = l->kf_tracked_ids[k]; }
    for (int k = nt; k < n; ++k) { l->h_kf_xy[2 * k] = l->h_tri_xy[2 * (k - nt)]; l->h_kf_xy[2 * k + 1] = l->h_tri_xy[2 * (k - nt) + 1]; l->h_kf_ids[k] = (long long)l->new_ids[k - nt]; }
    l->n = l->n_initial = n;
    l->from_host = true;
    l->last_pyr = PYR(li, i);  // clone of the image, :14 (the batch buffers are double-buffered: it stays valid through the next batch)
    l->last_l0 = L0(li, i);
    if (l->first_keyframe) { l->tvec[0] = l->tvec[1] = l->tvec[2] = 0.f; l->rvec[0] = l->rvec[1] = l->rvec[2] = 0.f; }  // :54-55
    res[i].is_keyframe = 1;
    res[i].n_new = kept;
    frame_done(li);
    return SVO_OK;
  }

  // PnP's verdict and pose out of the pinned mirrors: 0 = go on, -1 = error (set) or "launch again with all hypotheses" (queued)
  int consume_pnp(int li) {
    Lane* l = g->lanes[li];
    if (*l->h_bad) {
      ctx->err = "pipeline group: a tracked feature's entry of the landmark store belongs to another id (store capacity exceeded?)";
      error = SVO_ERR_CAPACITY;
      return -1;
    }
    l->best = *l->h_best;  // the launch's own RANSAC bookkeeping (csrc/pnp.hip pnp_group_kernel); -1: no model
    if (l->best == -2) {     // the adaptive cap stayed above the hypotheses of the first launch: all of them now
      l->pnp_all = true;
      enqueue(q_pnp, li, L_PNP_WAIT);
      return -1;
    }
    if (l->best >= 0) {
      double rv[3];
      svo_det_rvec_from_quat(l->h_out, rv);  // declared arithmetic (host/det_trig.h)
      for (int k = 0; k < 3; ++k) { l->rvec[k] = (float)rv[k]; l->tvec[k] = (float)l->h_out[4 + k]; }
      l->num_inliers = *l->h_nin;
    }
    return 0;
  }

  // after PnP (:84-134): keyframe pose, inlier copy; then dedup + sparse stereo + triangulation go out
  void after_pnp(int li, bool queue_tri = true) {
    Lane* l = g->lanes[li];
    svo_frame_result* res = &RES(li, 0);
    res[l->frame].n_inliers = l->num_inliers;
    svo_det_rodrigues_f(l->rvec, l->rmat);  // :84-85 cv::Rodrigues on a CV_32F rvec with declared arithmetic: the same bits on the host, on the device and in the oracle
    svo_det_quat_from_R(l->rmat, l->quat);  // :87-92
    const float* txy = l->h_xy[l->cur];
    const long long* tids = l->h_ids[l->cur];
    l->kf_tracked_ids.resize(l->num_inliers); l->kf_tracked_xy.resize(2 * (size_t)l->num_inliers);
    for (int k = 0; k < l->num_inliers; ++k) {  // :104-108
      const int idx = l->h_inl[k];
      l->kf_tracked_ids[k] = tids[idx];
      l->kf_tracked_xy[2 * k] = txy[2 * idx]; l->kf_tracked_xy[2 * k + 1] = txy[2 * idx + 1];
    }
    l->first_keyframe = false;
    if (queue_tri) enqueue(q_tri, li, L_TRI_WAIT);
  }

  // the keyframe path once the previous solve is joined (:71-82)
  int continue_keyframe(int li) {
    Lane* l = g->lanes[li];
    const int m = l->n;
    l->m_tracked = m;
    l->num_inliers = 0; l->best = -1;
    // :72 get_world_points: nothing to do on the host — the PnP launch reads the tracked features' world points from the lane's
    // device-resident landmark store, which the (joined) solve of the previous keyframe has written
    if (m >= MODEL) enqueue(q_pnp, li, L_PNP_WAIT);
    else after_pnp(li);
    return SVO_OK;
  }

  // the keyframe gate after tracking (:63-65)
  int after_track(int li) {
    Lane* l = g->lanes[li];
    svo_frame_result& r = RES(li, l->frame);
    const float av = *l->h_av;
    const float pl = (float)(1.0 - (double)((float)l->n / (float)l->n_initial));  // src/feature_tracker.cpp:64
    r.n_tracked = l->n; r.av_parallax = av; r.percent_lost = pl;
    if (av <= g->prm.parallax_thresh && (double)pl < svo_ref::KEYFRAME_PERCENT_LOST) { frame_done(li); return SVO_OK; }
    if (l->ba_state.load(std::memory_order_acquire) != BA_NONE) { l->state = L_NEED_SOLVE; EV(li, "need_solve", l->ba_state.load()); return SVO_OK; }
    return continue_keyframe(li);
  }

  int start_frame(int li) {
    Lane* l = g->lanes[li];
    const int i = l->frame;
    svo_frame_result& r = RES(li, i);
    const int n_det = hc[li * batch + i];
    r.n_detected = n_det;
    if (n_det < svo_ref::MIN_DETECTED) { frame_done(li); return SVO_OK; }  // :23-25
    if (!l->has_keyframe) {  // :30-58
      l->first_keyframe = true;
      l->num_inliers = 0;
      enqueue(q_tri, li, L_TRI_WAIT);
      return SVO_OK;
    }
    if (l->n <= 0) {  // nothing to track: the kernels would see n = 0 (host/pipeline.cpp: av_parallax = 0)
      l->n = 0; *l->h_av = 0.f;
      return after_track(li);
    }
    enqueue(q_track, li, L_TRACK_WAIT);
    return SVO_OK;
  }

  // one lane as far as the host alone can take it
  void advance_lane(int li) {
    Lane* l = g->lanes[li];
    for (bool again = true; again && !error;) {
      again = false;
      switch (l->state) {
        case L_IDLE:
          error = start_frame(li);
          progressed = true;
          again = l->state == L_IDLE;  // the frame ended on the host (too few corners / no keyframe gate): next frame
          break;
        case L_TRACK_WAIT:
          if (l->queued || !word_ready(l, W_TRACK)) break;
          EV(li, "track_done", l->frame);
          l->cur ^= 1; l->from_host = false;
          l->n = *l->h_n;
          l->last_pyr = PYR(li, l->frame);  // :66
          l->last_l0 = L0(li, l->frame);
          error = after_track(li);
          progressed = true; again = l->state == L_IDLE;
          break;
        case L_NEED_SOLVE:
          if (!solve_came_back(l)) break;
          EV(li, "solve_joined_for_pnp", l->frame);
          error = finish_solve(g, l);
          if (!error) error = continue_keyframe(li);
          progressed = true; again = l->state == L_IDLE;
          break;
        case L_PNP_WAIT:
          if (l->queued || !word_ready(l, W_PNP)) break;
          EV(li, "pnp_done", l->frame);
          progressed = true;
          if (consume_pnp(li) < 0) break;  // error, or all hypotheses are needed: queued again
          after_pnp(li, true);
          break;
        case L_TRI_WAIT:
          if (l->queued || !word_ready(l, W_TRI)) break;
          EV(li, "tri_done", l->frame);
          progressed = true;
          if (l->fused) {  // the launch rode behind the lane's PnP launch: PnP's results first (they are complete: same stream, earlier)
            l->fused = false;
            if (consume_pnp(li) < 0) break;  // (all hypotheses needed: the triangulation did nothing; both go out again)
            after_pnp(li, false);
          }
          error = keyframe_tail(li);
          again = l->state == L_IDLE;
          break;
        default: break;
      }
    }
  }

  // ================================================================ the stages of the driver
  // a1 on every frame of every lane + the pyramids (the reference detects on every frame, src/image_processor.cpp:22), the
  // corner counts on the host, and the capacity check
  int front_end() {
    const int mc = g->prm.max_corners;
    hipStream_t st = ctx->stream;
    bool tight = true;  // the lanes' images are one contiguous run: the batch-wide launches take all of them at once
    for (int l = 1; l < S; ++l) tight = tight && lbase[l] == lbase[0] + (size_t)l * batch * istride;
    const uint8_t* const left = lbase[0];
    const size_t lane_stride = istride * (size_t)batch;  // (of the contiguous case)
    for (int i = 0; i < ST_COUNT; ++i) { g->launches[i] = 0; g->lanes_carried[i] = 0; }
    g->pyr_cur ^= 1;  // the previous batch's pyramids stay valid: a lane's last tracked image lives there (src/feature_tracker.cpp:66)
    pyr = g->d_pyr[g->pyr_cur];
    int rc = SVO_OK;
    // ... but a lane that neither tracked nor made a keyframe during the WHOLE previous batch (every frame below MIN_DETECTED
    // corners, C-7; with batch = 1 one blank frame is enough) still holds its last image in the buffer that is rebuilt now:
    // the reference keeps a clone of it (src/feature_tracker.cpp:14,66), so the lane takes a private copy first (same stream
    // as the rebuild: ordered in front of it).
    const uint8_t* lo = pyr;
    const uint8_t* hi = pyr + g->pyr_stride * (size_t)g->n_lanes * (size_t)g->max_batch;
    for (Lane* l : g->lanes) {
      if (!l->last_pyr || l->last_pyr < lo || l->last_pyr >= hi) continue;
      SVO_HIP_CHECK(ctx, hipMemcpyAsync(l->d_own_pyr, l->last_pyr, g->pyr_stride, hipMemcpyDeviceToDevice, ctx->stream));
      l->last_pyr = l->d_own_pyr;  // level 0 was cloned into the pyramid at the end of the batch that produced it
      l->last_l0 = l->d_own_pyr;
    }
    if (tight) {
      rc = svo_corner_detect_batch_dev(ctx, left, S * batch, W, H, W, istride, mc, g->prm.quality, (double)g->prm.min_feature_distance, g->d_corners, g->d_ncorners);
      // level 0 of the pyramids is NOT copied: the tracker reads the caller's images in place (Pyr::l0) — except every lane's
      // last frame, which the next batch tracks from when the caller's buffer may hold other frames
      if (!rc) rc = svo_k_build_pyramid(ctx, left, S * batch, W, H, W, istride, pyr, g->pyr_stride, true);
      if (!rc) rc = svo_k_pyramid_level0(ctx, left + (size_t)(batch - 1) * istride, S, W, H, W, lane_stride, pyr + (size_t)(batch - 1) * g->pyr_stride,
                                         (size_t)batch * g->pyr_stride, st);
    } else {
      for (int l = 0; l < S && !rc; ++l) {
        rc = svo_corner_detect_batch_dev(ctx, lbase[l], batch, W, H, W, istride, mc, g->prm.quality, (double)g->prm.min_feature_distance,
                                         g->d_corners + (size_t)l * batch * 2 * mc, g->d_ncorners + (size_t)l * batch);
        if (!rc) rc = svo_k_build_pyramid(ctx, lbase[l], batch, W, H, W, istride, pyr + (size_t)l * batch * g->pyr_stride, g->pyr_stride, true);
        if (!rc) rc = svo_k_pyramid_level0(ctx, lbase[l] + (size_t)(batch - 1) * istride, 1, W, H, W, istride,
                                           pyr + ((size_t)l * batch + (size_t)(batch - 1)) * g->pyr_stride, g->pyr_stride, st);
      }
    }
    if (rc) return rc;
    g->launches[ST_FRONT_END] += 7; g->lanes_carried[ST_FRONT_END] += 7 * S;
    hc = g->h_counts;
    SVO_HIP_CHECK(ctx, hipMemcpyAsync(hc, g->d_ncorners, sizeof(int) * S * batch, hipMemcpyDeviceToHost, st));
    SVO_HIP_CHECK(ctx, hipMemcpyAsync(hc + S * batch, ctx->d_status, sizeof(int), hipMemcpyDeviceToHost, st));
    SVO_HIP_CHECK(ctx, hipStreamSynchronize(st));
    if (hc[S * batch]) {
      (void)hipMemsetAsync(ctx->d_status, 0, sizeof(int), st);
      ctx->err = (hc[S * batch] & 8) ? "corner detection: more raw local maxima than the streaming pass's list holds (raw_cap: width x height / 4 per image under a 1 GiB budget)"
                           : "corner detection exceeded a workspace bound (svo_limits.max_candidates)";
      return SVO_ERR_CAPACITY;
    }
    return SVO_OK;
  }

  // advance every lane as far as the host alone can
  void advance_lanes() {
    all_done = true;
    for (int li = 0; li < S && !error; ++li) {
      advance_lane(li);
      if (g->lanes[li]->state != L_DONE) all_done = false;
    }
  }

  // Launch discipline of the two stage families below: a stage's kernels go to an in-order stream, so a launch for ONE lane
  // right now would make the lane that is ready ten microseconds later queue behind it for a whole kernel duration (tracking:
  // 150-200 us) — measured: 8 lanes, 110 track launches for 120 lane-frames, 3,000 frames/s.  Instead a line launches only
  // while none of its launches is in flight; lanes that become ready meanwhile ride the next launch together (a bus, not
  // taxis).  Nobody waits for a lane that is not ready.  Which lanes ride which line and when a launch is ripe: host/group_lines.h.
  void scan_lines() {
    for (int i = 0; i < MAX_LINES; ++i) lk_busy[i] = chain_busy[i] = false;
    for (int li = 0; li < S; ++li) {
      const Lane* l = g->lanes[li];
      if (l->queued) continue;
      lk_busy[l->lk_line] |= l->state == L_TRACK_WAIT;
      chain_busy[l->chain_line] |= l->state == L_PNP_WAIT || l->state == L_TRI_WAIT;
    }
    t_now_us = now_us();
  }
  // the gather rule (SVO_GROUP_GATHER_US) for line `line` of a stage whose lanes come out of the launches of `near_state`
  bool ripe(const std::vector<int>& q, int line, int n_lines, int near_state) const {
    return svo_line_ripe(q, S, line, n_lines, t_now_us, g->gather_us, [&](int li) { return g->lanes[li]->t_q; },
                         [&](int li) { return g->lanes[li]->state == near_state && !g->lanes[li]->queued; });
  }

  void fill_lk_lane(Lane* l, int li, SvoLkLane& x, int workgroups) {
    const int nxt = l->cur ^ 1;
    x.pyr_prev = l->last_pyr; x.pyr_next = PYR(li, l->frame);
    x.l0_prev = l->last_l0; x.l0_next = L0(li, l->frame);
    x.xy = l->from_host ? l->h_kf_xy : l->d_xy[l->cur];
    x.init_xy = l->from_host ? l->h_kf_xy : l->d_init[l->cur];
    x.ids = l->from_host ? l->h_kf_ids : l->d_ids[l->cur];
    x.n = l->n;
    x.fwd = l->d_fwd; x.keep = l->d_keep; x.parallax = l->d_par;
    x.kept_xy = l->d_xy[nxt]; x.init_dst = l->d_init[nxt]; x.ids_dst = l->d_ids[nxt];
    x.host_xy = l->h_xy[nxt]; x.host_ids = l->h_ids[nxt]; x.host_n = l->h_n; x.host_av = l->h_av;
    l->arrive_total[C_LK] += (unsigned)workgroups;
    x.arrive = l->d_arrive + 16 * C_LK; x.arrive_target = l->arrive_total[C_LK];
    x.word = &l->words[16 * W_TRACK]; x.seq = ++l->seq[W_TRACK];
    l->queued = false;
  }

  // WHERE A TRACKING LAUNCH IS DECIDED: a free line takes the queued lanes it carries, once the gather rule lets it
  void launch_tracking() {
    scan_lines();
    for (int line = 0; line < g->n_lk && !error; ++line) {
      if (lk_busy[line] || !ripe(q_track, line, g->n_lk, L_TRI_WAIT)) continue;
      const std::vector<int> q_now = svo_line_take(q_track, line, g->n_lk);
      if (q_now.empty()) continue;
      for (int li : q_now) g->lanes[li]->lk_line = line;
      SvoLkLanes a;
      a.w = W; a.h = H;
      int gx = 1;
      for (int li : q_now) gx = std::max(gx, g->lanes[li]->n);
      a.map.per_chunk = 0; a.map.total = 0; a.map.chunks = 0;
      if (g->xcd_map) {
        int counts[SVO_MAX_LANES], j = 0;
        for (int li : q_now) counts[j++] = g->lanes[li]->n;
        svo_xcd_map_fill(a.map, counts, j, g->xcd_chunks);
      }
      int k = 0;
      for (int li : q_now) {
        Lane* l = g->lanes[li];
        fill_lk_lane(l, li, a.lane[k++], a.map.per_chunk > 0 ? std::max(1, l->n) : gx);
      }
      if ((error = svo_kg_track(ctx, g->st_lk[line], a, k, gx))) return;
      for (int li : q_now) EV(li, "track_launch", k);
      count(ST_TRACK, k);
    }
  }

  void fill_pnp_lane(Lane* l, int li, SvoPnpLane& x) {
    (void)li;
    const int m = l->m_tracked;
    x.ids = l->d_ids[l->cur]; x.store = l->d_store; x.store_mask = l->store_mask;
    x.xy = l->d_xy[l->cur]; x.n = m;
    x.f = (double)g->K[0]; x.cx = (double)g->K[2]; x.cy = (double)g->K[5];
    // rvec/tvec are CV_32F in/out, the solver works in double (host/pipeline.cpp; csrc/pnp.hip svo_k_pnp)
    const double rv[3] = {l->rvec[0], l->rvec[1], l->rvec[2]};
    svo_det_quat_from_rvec(rv, x.q0);  // declared arithmetic (host/det_trig.h)
    for (int c = 0; c < 3; ++c) x.t0[c] = (double)l->tvec[c];
    x.thr2 = (double)svo_ref::PNP_REPROJ_ERROR * (double)svo_ref::PNP_REPROJ_ERROR;
    x.confidence = svo_ref::PNP_CONFIDENCE; x.iterations = g->pnp_iterations;
    x.launched = l->pnp_all ? g->pnp_iterations : svo_kg_pnp_first(g->pnp_iterations);
    l->pnp_all = false;
    const int wgs = svo_kg_pnp_workgroups(x.launched);
    x.hyp_pose = l->d_hyp_pose; x.hyp_count = l->d_hyp_count; x.hyp_mask = l->d_hyp_mask; x.mask_words = svo_div_up(m, 64);
    x.out_pose = l->d_out; x.inliers = l->d_inl; x.n_inliers = l->d_nin; x.inlier_xy = l->d_trk_xy;
    x.host_pose = l->h_out; x.host_inliers = l->h_inl; x.host_nin = l->h_nin; x.host_best = l->h_best; x.host_bad = l->h_bad;
    const SvoPublish pb = make_pub(l, W_PNP, C_PNP, wgs);
    x.arrive = pb.arrive; x.arrive_target = pb.target; x.word = pb.word; x.seq = pb.seq;
    // fused chain: the launch leaves M / the inlier count / "more hypotheses first" for the stereo launch right behind it
    x.chain = chain_fused ? l->d_chain : nullptr;
    for (int c = 0; c < 3; ++c) { x.prev_rvec[c] = l->rvec[c]; x.prev_tvec[c] = l->tvec[c]; }
    x.cam_f = g->K[0]; x.cam_cx = g->K[2]; x.cam_cy = g->K[5]; x.cam_b = (float)g->prm.cam.baseline;
    l->queued = false;
  }

  // the PnP launch of a chain line; with the fused chain its lanes join t_now: their stereo launch rides right behind
  void launch_pnp(int line, const std::vector<int>& h_now, std::vector<int>& t_now) {
    SvoPnpLanes a;
    int k = 0;
    for (int li : h_now) fill_pnp_lane(g->lanes[li], li, a.lane[k++]);
    if ((error = svo_kg_pnp(ctx, g->st_chain[line], a, k))) return;
    for (int li : h_now) EV(li, "pnp_launch", k);
    count(ST_PNP, k);
    if (chain_fused) for (int li : h_now) { g->lanes[li]->fused = true; t_now.push_back(li); }
  }

  void fill_tri_lane(Lane* l, int li, SvoStereoTriLane& x, int workgroups) {
    const int i = l->frame, n_det = hc[li * batch + i];
    x.xy = DET(li, i); x.n_dev = nullptr;
    x.trk = nullptr; x.n_trk = 0; x.min_d = 0.f;
    x.chain = nullptr;
    if (l->fused) {  // behind the lane's PnP launch: M and the inlier count are read from its record on the device
      x.chain = l->d_chain; x.trk = l->d_trk_xy; x.min_d = g->prm.min_feature_distance;
    } else if (!l->first_keyframe) {
      // dedup (:113-128) inside the same launch: every corner's workgroup tests it against the tracked inliers first
      x.trk = l->d_trk_xy; x.n_trk = l->num_inliers; x.min_d = g->prm.min_feature_distance;
      if (x.n_trk <= 0) x.trk = nullptr;  // no inliers (C-9): nothing to keep away from
    }
    x.left = IMG(lbase, li, i); x.right = IMG(rbase, li, i);
    x.n_max = n_det; x.disp = l->d_disp;
    // :130-134, :178-189: M = float(hmat * Q), hmat = [R^T | -R^T t] of the keyframe's pose (host/chain_math.h) — of the identity
    // for frame 0 and for a fused lane, which reads M from the device record instead
    const float I9[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, zero3[3] = {0, 0, 0};
    const bool posed = !l->fused && !l->first_keyframe;
    svo_chain_matrix_from_R(posed ? l->rmat : I9, posed ? l->tvec : zero3, g->K[0], g->K[2], g->K[5], (float)g->prm.cam.baseline, x.M.m);
    x.kept_xy = l->h_tri_xy; x.xyz = l->h_tri_xyz; x.n_kept = l->h_tri_cnt;
    x.pub = make_pub(l, W_TRI, C_TRI, workgroups);
    l->state = L_TRI_WAIT;
    l->queued = false;
  }

  // dedup (:113-128) for the lanes that tracked, then sparse StereoBM + triangulation (:137-142, :34-39 for frame 0)
  void launch_tri(int line, const std::vector<int>& t_now) {
    SvoStereoTriLanes t;
    t.w = W; t.h = H; t.stride = W; t.ndisp = svo_ref::STEREO_NUM_DISPARITIES; t.block = svo_ref::STEREO_BLOCK_SIZE;
    int kt = 0, gxt = 1;
    t.map.per_chunk = 0; t.map.total = 0; t.map.chunks = 0;
    int counts[SVO_MAX_LANES], j = 0;
    for (int li : t_now) {
      const int n_det = hc[li * batch + g->lanes[li]->frame];
      gxt = std::max(gxt, n_det);
      counts[j++] = n_det;
    }
    if (g->xcd_map_tri) svo_xcd_map_fill(t.map, counts, j, g->xcd_chunks);
    for (int li : t_now) {
      Lane* l = g->lanes[li];
      fill_tri_lane(l, li, t.lane[kt++], t.map.per_chunk > 0 ? std::max(1, hc[li * batch + l->frame]) : gxt);
    }
    if ((error = svo_kg_stereo_triangulate(ctx, g->st_chain[line], t, kt, gxt))) return;
    for (int li : t_now) EV(li, "tri_launch", kt);
    count(ST_TRI, kt);
  }

  // the keyframe chains: per free chain line one PnP launch (under the gather rule) and one stereo + triangulation launch
  void launch_chains() {
    for (int line = 0; line < g->n_chain && !error; ++line) {
      if (chain_busy[line]) continue;
      const std::vector<int> h_now = ripe(q_pnp, line, g->n_chain, L_TRACK_WAIT) ? svo_line_take(q_pnp, line, g->n_chain) : std::vector<int>();
      std::vector<int> t_now = svo_line_take(q_tri, line, g->n_chain);
      for (int li : h_now) g->lanes[li]->chain_line = line;
      for (int li : t_now) g->lanes[li]->chain_line = line;
      if (!h_now.empty()) launch_pnp(line, h_now, t_now);
      if (!error && !t_now.empty()) launch_tri(line, t_now);
    }
  }

  // (a solve that stepped aside has not come back: it is joined as such here — budget back, line free once the launch's other words
  // are out — and waits for the group's next wide launch, in front of the solves that have never run)
  bool solve_came_back(Lane* l) {
    const int bs = l->ba_state.load(std::memory_order_acquire);
    if (bs == BA_INFLIGHT && svo_ba_solve_poll(l->ba) && svo_ba_solve_continues(l->ba)) {
      l->ba_yielded = true;
      l->ba_state.store(BA_READY, std::memory_order_release);
      progressed = true;
      return false;
    }
    return (bs == BA_INFLIGHT && svo_ba_solve_poll(l->ba)) || bs == BA_HOST_DONE;
  }
  bool any_solve_in_flight(bool holding_budget) const {
    bool any = false;
    for (const Lane* l : g->lanes)
      any |= l->ba_state.load(std::memory_order_acquire) == BA_INFLIGHT && (!holding_budget || svo_ba_solve_holds_budget(l->ba));
    return any;
  }

  // A finished solve is joined right away (its admission is handed back: lanes that are already through their frames would
  // otherwise keep the budget while others wait for it); the results are the same whenever they are read.
  void join_finished_solves() {
    for (int li = 0; li < S && !error; ++li) {
      Lane* l = g->lanes[li];
      if (l->state == L_NEED_SOLVE || !solve_came_back(l)) continue;  // (a lane in L_NEED_SOLVE joins its own: advance_lane)
      EV(li, "solve_joined", l->frame);
      error = finish_solve(g, l);
      progressed = true;
    }
  }

  // THE ONE PLACE WHERE A SOLVE BECOMES IN FLIGHT: a solve launch has left on solve line `line`; it carries the `carried`
  // lanes of lanes[0..n) whose bit is set in `taken`
  void solves_departed(const int* lanes, int n, unsigned long long taken, int line, int carried, const char* what) {
    ++g->ba_launch_id;
    int fresh = 0;  // (a solve is counted once: with its first launch)
    for (int k = 0; k < n; ++k) fresh += ((taken >> k) & 1ull) && !g->lanes[lanes[k]]->ba_yielded;
    if (fresh > 0) count(ST_SOLVE, fresh);
    else if (carried > 0) progressed = true;
    for (int k = 0; k < n; ++k) {
      if (!((taken >> k) & 1ull)) continue;
      Lane* l = g->lanes[lanes[k]];
      EV(lanes[k], what, carried);
      l->ba_launch = g->ba_launch_id; l->ba_line = line;  // (ba_ready_seq stays until the join: a solve that steps aside keeps its place)
      l->ba_state.store(BA_INFLIGHT, std::memory_order_release);
    }
  }
  static int first_not_taken(const int* lanes, int n, unsigned long long taken) {
    for (int k = 0; k < n; ++k) if (!((taken >> k) & 1ull)) return lanes[k];
    return -1;
  }

  // the assembled solves in the order of their admission (host/group_lines.h), and which solve lines are busy
  void collect_ready_solves() {
    q_ba.clear();
    for (int li = 0; li < S; ++li) {
      Lane* l = g->lanes[li];
      if (l->ba_state.load(std::memory_order_acquire) != BA_READY) continue;
      q_ba.push_back(li);
      if (!l->ba_ready_seq) l->ba_ready_seq = ++g->ba_ready_counter;
    }
    std::sort(q_ba.begin(), q_ba.end(), [&](int a, int b) {
      const Lane* la = g->lanes[a]; const Lane* lb = g->lanes[b];
      return svo_solve_before(la->state == L_NEED_SOLVE, la->ba_yielded, la->ba_ready_seq, lb->state == L_NEED_SOLVE, lb->ba_yielded, lb->ba_ready_seq);
    });
    for (int i = 0; i < MAX_LINES; ++i) ba_line_busy[i] = false;
    for (const Lane* l : g->lanes)
      if (l->ba_state.load(std::memory_order_acquire) == BA_INFLIGHT && !svo_ba_solve_poll(l->ba)) ba_line_busy[l->ba_line] = true;
  }
  int free_solve_line(int from, int to) const {
    for (int i = from; i < to; ++i) if (!ba_line_busy[i]) return i;
    return -1;
  }

  // compact lines (SVO_GROUP_COMPACT_LINES, round 5): what the admission budget refused while nothing of this group holds any
  // of it leaves at once in the one-workgroup form — no budget, 3-4x the latency — on a line of its own, so that the wide
  // launches' lines stay free.  Returns the first lane that is still not taken (-1: none).
  int launch_refused_compact(const int* cand, svo_ba* const* bas, int n, unsigned long long mask, int not_taken) {
    const int cline = free_solve_line(g->n_ba, g->n_ba + g->n_cmp);
    if (cline < 0) return not_taken;
    svo_ba* cb[SVO_MAX_LANES];
    int cl[SVO_MAX_LANES], nc = 0;
    for (int k = 0; k < n; ++k) if (!((mask >> k) & 1ull) && !g->lanes[cand[k]]->ba_yielded) { cb[nc] = bas[k]; cl[nc++] = cand[k]; (void)svo_ba_set_solve_form(bas[k], 1); }
    unsigned long long cmask = 0;
    const int went = nc ? svo_ba_solve_launch(cb, nc, g->st_ba[cline], &cmask) : 0;  // (a solve that stepped aside stays wide: it waits)
    for (int k = 0; k < nc; ++k) (void)svo_ba_set_solve_form(cb[k], -1);
    if (went <= 0) return not_taken;
    solves_departed(cl, nc, cmask, cline, went, "ba_launch_compact");
    return first_not_taken(cl, nc, cmask);
  }

  // Everything that has been assembled goes out as ONE wide launch on a free solve line, at once (rounds 3-4 held ready solves
  // back while any lane was still assembling, to launch them together: measured in round 4, a solve then left 1.1 ms after its
  // assembly was posted on average — as long as it runs — and 3 ms at the 90th percentile).
  // WHERE A REFUSED SOLVE GOES: the three cases at the end of this function.
  void launch_solves() {
    collect_ready_solves();
    const int free_line = free_solve_line(0, g->n_ba);
    if (q_ba.empty() || free_line < 0) return;
    svo_ba* bas[SVO_MAX_LANES];
    int cand[SVO_MAX_LANES], n = 0;
    for (int li : q_ba) {
      Lane* l = g->lanes[li];
      if (l->ba_rc == 1) { l->ba_ready_seq = 0; l->ba_state.store(BA_NONE, std::memory_order_release); continue; }  // nothing to solve
      if (l->ba_rc) { error = l->ba_rc; return; }
      bas[n] = l->ba;
      cand[n++] = li;
    }
    if (!n) return;
    unsigned long long mask = 0;
    const bool host_solves = host_solves_only();
    const int launched = host_solves ? 0 : svo_ba_solve_launch(bas, n, g->st_ba[free_line], &mask);
    solves_departed(cand, n, mask, free_line, launched, "ba_launch");
    int not_taken = first_not_taken(cand, n, mask);  // the first lane the launch skipped: not eligible, or not admitted right now
    if (not_taken < 0) return;
    // 1. A refused solve waits for the group's next wide launch while a wide solve of this group is in flight: joining it hands
    // budget back, the solve is offered again in the next pass (at a larger k if need be, ba_device_lm_launch) and rides a launch
    // that costs the same queue time with or without it — one workgroup for 6 ms holds a hardware queue that the tracking line
    // shares (4 queues: 12.25 against 12.05 k frames/s at 96 lanes, profiles/r08_runs.txt).
    // 2. Nothing of the group holds budget and it has compact lines: the refused solves leave in the compact form.
    if (g->n_cmp > 0 && !host_solves && !any_solve_in_flight(true)) not_taken = launch_refused_compact(cand, bas, n, mask, not_taken);
    // 3. Nothing of this group is in flight that could free the admission budget (or the problem is simply not eligible for
    // the device-resident solve): the lane is solved by the host-driven loop on a worker (a compact solve here instead was
    // measured slower, 29 k against 41 k frames/s at 128 lanes, profiles/r05_exp_lanes_groups.txt: it holds its solve line
    // for ~3 ms, the worker holds none).  Otherwise it is offered again when a solve of this group has been joined.
    if (not_taken < 0 || any_solve_in_flight(false)) return;
    Lane* l = g->lanes[not_taken];
    l->ba_ready_seq = 0;
    l->ba_state.store(BA_HOST_SOLVING, std::memory_order_release);
    g->pool.post(l, 1);
    progressed = true;
  }

  // a pass that moved nothing: spin politely, and never hang — a launch that does not come back within seconds is reported
  // with the lanes' states.  False: give up (error is set).
  bool idle_or_report() {
    if (progressed) {
      idle_spins = 0;
      last_progress = Clock::now();
      busy_us += std::chrono::duration<double, std::micro>(last_progress - t_pass).count();
      return true;
    }
    __builtin_ia32_pause();
    if (++idle_spins > 2000u && (idle_spins & 255u) == 0) sched_yield();
    if ((idle_spins & 0xFFFFu) != 0) return true;
    if (std::chrono::duration<double>(Clock::now() - last_progress).count() <= 5.0) return true;
    std::string msg = "pipeline group: no progress for 5 s; lanes (state/frame/solve):";
    for (const Lane* l : g->lanes) {
      char b[64];
      snprintf(b, sizeof(b), " %d/%d/%d%s", l->state, l->frame, l->ba_state.load(), l->queued ? "q" : "");
      msg += b;
    }
    ctx->err = msg;
    error = SVO_ERR_HIP;
    return false;
  }

  // a lane whose assembly is still running at the end of the batch, or whose solve is not launched yet: see it launched
  void launch_last_solve(int li) {
    Lane* l = g->lanes[li];
    for (;;) {
      const int bs = l->ba_state.load(std::memory_order_acquire);
      if (bs == BA_NONE || bs == BA_INFLIGHT || bs == BA_HOST_DONE) return;
      if (bs == BA_READY) {
        if (l->ba_rc) {  // 1: nothing to solve
          if (l->ba_rc != 1 && !error) error = l->ba_rc;
          l->ba_state.store(BA_NONE);
          return;
        }
        svo_ba* one = l->ba;
        if (svo_ba_solve_launch(&one, 1, g->st_ba[0], nullptr) == 1) solves_departed(&li, 1, 1ull, 0, 1, "ba_launch_at_end");
        else { l->ba_rc = svo_ba_solve_finish(l->ba, &l->ba_summary); l->ba_state.store(BA_HOST_DONE); }
        return;
      }
      __builtin_ia32_pause();
      if (std::chrono::duration<double>(Clock::now() - last_progress).count() > 60.0) {
        if (!error) { error = SVO_ERR_HIP; ctx->err = "pipeline group: a bundle-adjustment worker did not come back"; }
        return;
      }
    }
  }

  // A lane whose last tracked image is NOT the batch's last frame (its later frames had too few corners to track, C-7)
  // still reads that image's level 0 from the caller's buffer: clone it into its pyramid now (src/feature_tracker.cpp:14,66),
  // before the caller may reuse the buffer.
  void clone_last_level0() {
    hipStream_t st = ctx->stream;
    bool copied = false;
    for (int li = 0; li < S && !error; ++li) {
      Lane* l = g->lanes[li];
      if (!l->last_pyr || l->last_l0 == l->last_pyr || !l->last_l0) continue;
      if (svo_k_pyramid_level0(ctx, l->last_l0, 1, W, H, W, istride, const_cast<uint8_t*>(l->last_pyr), g->pyr_stride, st)) { error = SVO_ERR_HIP; break; }
      l->last_l0 = l->last_pyr;
      copied = true;
    }
    if (copied && hipStreamSynchronize(st) != hipSuccess && !error) { error = SVO_ERR_HIP; ctx->err = "pipeline group: pyramid clone failed"; }
  }

  // end of the batch: join every solve, fill the poses that waited for it
  int end_of_batch() {
    g->launches[ST_HOST_US] += (long)busy_us;
    g->lanes_carried[ST_HOST_US] += (long)now_us();
    for (int li = 0; li < S; ++li) {
      Lane* l = g->lanes[li];
      launch_last_solve(li);
      const int rcf = finish_solve(g, l);
      if (rcf && !error) error = rcf;
      if (l->pending_from < 0) l->pending_from = batch;
      fill_pending(l, &RES(li, 0), batch);
    }
    clone_last_level0();
    if (trace_on) {
      static std::mutex trace_mu;  // the groups of a process print their calls one after the other
      std::lock_guard<std::mutex> lk(trace_mu);
      for (const Ev& e : evs) fprintf(stderr, "[svo group] %10.1f lane %2d %-22s %d\n", e.us, e.lane, e.what, e.arg);
      fprintf(stderr, "[svo group] %10.1f end\n", now_us());
    }
    if (error) { quiesce_after_error(g); return error; }
    if (!ctx->err.empty()) return SVO_ERR_HIP;
    return SVO_OK;
  }

  int run() {
    const int rc = front_end();
    if (rc) return rc;
    for (int li = 0; li < S; ++li) {
      Lane* l = g->lanes[li];
      l->frame = 0; l->state = L_IDLE; l->queued = false; l->pending_from = -1;
      memset(&RES(li, 0), 0, sizeof(svo_frame_result) * batch);
    }
    t_begin = last_progress = Clock::now();
    for (;;) {
      progressed = false;
      t_pass = Clock::now();
      advance_lanes();
      if (!error) launch_tracking();
      if (!error) launch_chains();
      if (!error) join_finished_solves();
      if (!error) launch_solves();
      if (error || all_done || !idle_or_report()) break;
    }
    return end_of_batch();
  }
};

int group_process(svo_pipeline_group* g, const uint8_t* const* lbase, const uint8_t* const* rbase, int batch, svo_frame_result* results) {
  return Batch(g, lbase, rbase, batch, results).run();
}
}  // namespace

extern "C" int svo_pipeline_group_process_batch_dev(svo_pipeline_group* g, const uint8_t* left, const uint8_t* right, size_t lane_stride,
                                                    int batch, svo_frame_result* results) {
  if (!g) return SVO_ERR_INVALID;
  svo_ctx* ctx = g->ctx;
  SVO_REQUIRE(ctx, left && right && results && batch >= 1 && batch <= g->max_batch, "pipeline_group_process_batch: bad arguments");
  const int W = g->prm.width, H = g->prm.height, S = g->n_lanes;
  const size_t istride = (size_t)W * H;
  SVO_REQUIRE(ctx, lane_stride >= istride * (size_t)batch, "pipeline_group_process_batch: lanes overlap");
  ctx->err.clear();
  SVO_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if (g->kfc) svo_kfc_clear(g->kfc);  // the table of the previous call ends here
  const uint8_t *lbase[SVO_MAX_LANES], *rbase[SVO_MAX_LANES];
  for (int l = 0; l < S; ++l) { lbase[l] = left + (size_t)l * lane_stride; rbase[l] = right + (size_t)l * lane_stride; }
  // raw input: ONE remap launch for every lane that has a camera model, in front of everything (same stream as the batch-wide
  // stages); those lanes are then read from the workspace (lanes `batch` images apart: contiguous when every lane is rectified).
  // A lane without a model is neither remapped nor copied.
  if (!g->rect_models.empty()) {
    SvoRectifyArgs a{};
    const size_t ws_lane = istride * (size_t)batch;
    a.src[0] = left; a.src[1] = right; a.dst[0] = g->d_rect[0]; a.dst[1] = g->d_rect[1];
    a.src_lane_stride = lane_stride; a.dst_lane_stride = ws_lane;
    a.src_image_stride = a.dst_image_stride = istride;
    a.src_row_stride = W; a.width = W; a.height = H; a.frames = batch; a.eyes = 2;
    for (int l = 0; l < S; ++l) {
      const SvoRectModel* m = g->lane_rect[l];
      if (!m) continue;
      a.map[a.n_active][0] = m->d_map[0]; a.map[a.n_active][1] = m->d_map[1];
      a.lane[a.n_active++] = (unsigned char)l;
      lbase[l] = g->d_rect[0] + (size_t)l * ws_lane; rbase[l] = g->d_rect[1] + (size_t)l * ws_lane;
    }
    if (a.n_active) {
      const int rc = svo_k_rectify_remap(ctx, a, ctx->stream);
      if (rc) return rc;
    }
  }
  const int rc = group_process(g, lbase, rbase, batch, results);
  if (rc || !g->kfc) return rc;
  // keyframe clouds: the event loop has drained and every lane's frames are finished; the images (a rectified lane's: its
  // workspace copies) are still resident.  ONE dense launch + ONE cloud launch sequence for all (lane, frame) keyframes of
  // the lanes that have clouds on — nothing of this lives in the loop's state machines.
  std::vector<SvoCloudPair> pairs;
  std::vector<int> frame, lane;
  for (int l = 0; l < S; ++l) {
    if (!g->lane_cloud[l]) continue;
    for (int i = 0; i < batch; ++i)
      if (results[(size_t)l * batch + i].is_keyframe) {
        pairs.push_back({lbase[l] + (size_t)i * istride, rbase[l] + (size_t)i * istride});
        frame.push_back(i); lane.push_back(l);
      }
  }
  return svo_kfc_run(g->kfc, &g->prm.cam, pairs.data(), frame.data(), lane.data(), (int)frame.size());
}

extern "C" int svo_pipeline_group_set_keyframe_clouds(svo_pipeline_group* g, int lane, const svo_cloud_params* params, int max_keyframes_per_call) {
  if (!g) return SVO_ERR_INVALID;
  svo_ctx* ctx = g->ctx;
  SVO_REQUIRE(ctx, lane >= -1 && lane < g->n_lanes, "pipeline_group_set_keyframe_clouds: no such lane");
  SVO_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  bool others = false;  // lanes outside this call's selection that have clouds on
  for (int l = 0; l < g->n_lanes; ++l) others = others || (g->lane_cloud[l] && lane >= 0 && l != lane);
  if (params) {
    bool same = false;
    if (g->kfc) {
      const svo_cloud_params* have = svo_kfc_params(g->kfc);
      const int want_points = kfc_max_points(params->max_points, g->prm.width, g->prm.height);
      const int want_kf = kfc_max_keyframes(max_keyframes_per_call, ctx->lim.max_batch);
      same = have->step == params->step && have->min_disparity == params->min_disparity && have->max_points == want_points &&
             svo_kfc_max_keyframes(g->kfc) == want_kf;
    }
    SVO_REQUIRE(ctx, same || !others, "pipeline_group_set_keyframe_clouds: the lanes that have clouds on share one set of parameters and one bound");
    if (!same) {
      const int rc = svo_kfc_replace(ctx, &g->kfc, params, g->prm.width, g->prm.height, max_keyframes_per_call);  // the switches that were on stay on
      if (rc) return rc;
    }
  }
  for (int l = 0; l < g->n_lanes; ++l)
    if (lane < 0 || l == lane) g->lane_cloud[l] = params != nullptr;
  bool any = false;
  for (int l = 0; l < g->n_lanes; ++l) any = any || g->lane_cloud[l];
  if (!any) { svo_kfc_destroy(g->kfc); g->kfc = nullptr; }  // the last lane turned off: everything goes
  return SVO_OK;
}

extern "C" int svo_pipeline_group_set_keyframe_speckle_filter(svo_pipeline_group* g, const svo_speckle_params* params) {
  if (!g) return SVO_ERR_INVALID;
  SVO_HIP_CHECK(g->ctx, hipSetDevice(g->ctx->device));
  SVO_REQUIRE(g->ctx, g->kfc, "pipeline_group_set_keyframe_speckle_filter: keyframe clouds are off on every lane (call svo_pipeline_group_set_keyframe_clouds first)");
  return svo_kfc_set_speckle(g->kfc, params);
}

extern "C" int svo_pipeline_group_set_keyframe_lr_check(svo_pipeline_group* g, const svo_lr_check_params* params) {
  if (!g) return SVO_ERR_INVALID;
  SVO_HIP_CHECK(g->ctx, hipSetDevice(g->ctx->device));
  SVO_REQUIRE(g->ctx, g->kfc, "pipeline_group_set_keyframe_lr_check: keyframe clouds are off on every lane (call svo_pipeline_group_set_keyframe_clouds first)");
  return svo_kfc_set_lr_check(g->kfc, params);
}

extern "C" int svo_pipeline_group_set_keyframe_sgm(svo_pipeline_group* g, const svo_sgm_params* params) {
  if (!g) return SVO_ERR_INVALID;
  SVO_HIP_CHECK(g->ctx, hipSetDevice(g->ctx->device));
  SVO_REQUIRE(g->ctx, g->kfc, "pipeline_group_set_keyframe_sgm: keyframe clouds are off on every lane (call svo_pipeline_group_set_keyframe_clouds first)");
  return svo_kfc_set_sgm(g->kfc, params);
}

extern "C" int svo_pipeline_group_keyframe_clouds(svo_pipeline_group* g, int* n, const svo_keyframe_cloud** table) {
  if (!g || !n) return SVO_ERR_INVALID;
  *n = 0;
  if (table) *table = nullptr;
  SVO_REQUIRE(g->ctx, g->kfc, "pipeline_group_keyframe_clouds: keyframe clouds are off on every lane");
  return svo_kfc_table(g->kfc, n, table);
}

extern "C" int svo_pipeline_group_copy_keyframe_cloud(svo_pipeline_group* g, int i, svo_cloud_point* host, int capacity) {
  if (!g) return SVO_ERR_INVALID;
  SVO_REQUIRE(g->ctx, g->kfc, "pipeline_group_copy_keyframe_cloud: keyframe clouds are off on every lane");
  return svo_kfc_copy(g->kfc, i, host, capacity);
}

extern "C" int svo_pipeline_group_keyframe_disparity(svo_pipeline_group* g, int i, const int16_t** dev) {
  if (!g) return SVO_ERR_INVALID;
  SVO_REQUIRE(g->ctx, g->kfc, "pipeline_group_keyframe_disparity: keyframe clouds are off on every lane");
  return svo_kfc_disparity(g->kfc, i, dev);
}

extern "C" int svo_pipeline_group_copy_keyframe_disparity(svo_pipeline_group* g, int i, int16_t* host) {
  if (!g) return SVO_ERR_INVALID;
  SVO_REQUIRE(g->ctx, g->kfc, "pipeline_group_copy_keyframe_disparity: keyframe clouds are off on every lane");
  return svo_kfc_copy_disparity(g->kfc, i, host);
}

// Raw input per lane (include/svo.h).  The tables of a (left, right) pair of models exist once, however many lanes use it.
extern "C" int svo_pipeline_group_set_rectification(svo_pipeline_group* g, int lane, const svo_rectify_eye* left, const svo_rectify_eye* right) {
  if (!g) return SVO_ERR_INVALID;
  svo_ctx* ctx = g->ctx;
  SVO_REQUIRE(ctx, lane >= -1 && lane < g->n_lanes, "pipeline_group_set_rectification: no such lane");
  SVO_REQUIRE(ctx, (left != nullptr) == (right != nullptr), "pipeline_group_set_rectification: give both eyes, or neither to turn it off");
  SVO_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  SvoRectModel* m = nullptr;
  if (left) {
    for (SvoRectModel* have : g->rect_models)
      if (!memcmp(&have->eye[0], left, sizeof(*left)) && !memcmp(&have->eye[1], right, sizeof(*right))) m = have;
    if (!m) {
      const int rc = svo_rect_model_create(ctx, left, right, &g->prm.cam, g->prm.width, g->prm.height, &m);
      if (rc) return rc;
      g->rect_models.push_back(m);
    }
    const size_t bytes = (size_t)g->n_lanes * (size_t)g->max_batch * (size_t)g->prm.width * (size_t)g->prm.height;
    for (int e = 0; e < 2; ++e)
      if (!g->d_rect[e]) SVO_HIP_CHECK(ctx, hipMalloc((void**)&g->d_rect[e], bytes));
  }
  for (int l = 0; l < g->n_lanes; ++l) {
    if (lane >= 0 && l != lane) continue;
    if (g->lane_rect[l]) --g->lane_rect[l]->refs;
    g->lane_rect[l] = m;
    if (m) ++m->refs;
  }
  // tables no lane uses any more go; with the last one the workspace goes too (process_batch* returns with its launches complete)
  for (size_t i = 0; i < g->rect_models.size();) {
    if (g->rect_models[i]->refs > 0) { ++i; continue; }
    svo_rect_model_destroy(g->rect_models[i]);
    g->rect_models.erase(g->rect_models.begin() + (long)i);
  }
  if (g->rect_models.empty())
    for (int e = 0; e < 2; ++e) { if (g->d_rect[e]) (void)hipFree(g->d_rect[e]); g->d_rect[e] = nullptr; }
  return SVO_OK;
}

// ---- host-pointer / streaming entry (include/svo.h): the reference's images are host cv::Mat copies made in the image
// callback (src/vo_node.cpp:70-73) and consumed frame by frame (:141-143)
namespace {
int ensure_staging(svo_pipeline_group* g) {
  if (g->st_copy) return SVO_OK;
  svo_ctx* ctx = g->ctx;
  SVO_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const size_t bytes = (size_t)g->n_lanes * (size_t)g->max_batch * (size_t)g->prm.width * (size_t)g->prm.height;
  // only what is still missing: a call that failed half way (out of pinned memory) leaves st_copy null and comes back here
  for (int sl = 0; sl < 2; ++sl) {
    for (int e = 0; e < 2; ++e) {
      if (!g->h_stage[sl][e]) SVO_HIP_CHECK(ctx, hipHostMalloc((void**)&g->h_stage[sl][e], bytes, hipHostMallocDefault));
      if (!g->d_stage[sl][e]) SVO_HIP_CHECK(ctx, hipMalloc((void**)&g->d_stage[sl][e], bytes));
    }
    if (!g->ev_up[sl]) SVO_HIP_CHECK(ctx, hipEventCreateWithFlags(&g->ev_up[sl], hipEventDisableTiming));
  }
  SVO_HIP_CHECK(ctx, hipStreamCreateWithFlags(&g->st_copy, hipStreamNonBlocking));
  return SVO_OK;
}
}  // namespace

extern "C" int svo_pipeline_group_staging(svo_pipeline_group* g, int slot, uint8_t** left, uint8_t** right, size_t* lane_stride) {
  if (!g || slot < 0 || slot > 1 || !left || !right) return SVO_ERR_INVALID;
  const int rc = ensure_staging(g);
  if (rc) return rc;
  *left = g->h_stage[slot][0]; *right = g->h_stage[slot][1];
  if (lane_stride) *lane_stride = (size_t)g->max_batch * (size_t)g->prm.width * (size_t)g->prm.height;
  return SVO_OK;
}

extern "C" int svo_pipeline_group_upload(svo_pipeline_group* g, int slot, int batch) {
  if (!g || slot < 0 || slot > 1) return SVO_ERR_INVALID;
  svo_ctx* ctx = g->ctx;
  SVO_REQUIRE(ctx, batch >= 1 && batch <= g->max_batch, "pipeline_group_upload: batch outside 1..max_batch");
  int rc = ensure_staging(g);
  if (rc) return rc;
  SVO_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const size_t istride = (size_t)g->prm.width * (size_t)g->prm.height, lane_bytes = (size_t)g->max_batch * istride;
  for (int e = 0; e < 2; ++e) {
    if (batch == g->max_batch)  // one contiguous run
      SVO_HIP_CHECK(ctx, hipMemcpyAsync(g->d_stage[slot][e], g->h_stage[slot][e], lane_bytes * (size_t)g->n_lanes, hipMemcpyHostToDevice, g->st_copy));
    else                        // the first `batch` frames of every lane
      SVO_HIP_CHECK(ctx, hipMemcpy2DAsync(g->d_stage[slot][e], lane_bytes, g->h_stage[slot][e], lane_bytes, (size_t)batch * istride, (size_t)g->n_lanes,
                                          hipMemcpyHostToDevice, g->st_copy));
  }
  SVO_HIP_CHECK(ctx, hipEventRecord(g->ev_up[slot], g->st_copy));
  g->up_batch[slot] = batch;
  return SVO_OK;
}

extern "C" int svo_pipeline_group_process_uploaded(svo_pipeline_group* g, int slot, svo_frame_result* results) {
  if (!g || slot < 0 || slot > 1) return SVO_ERR_INVALID;
  svo_ctx* ctx = g->ctx;
  SVO_REQUIRE(ctx, g->st_copy && g->up_batch[slot] > 0, "pipeline_group_process_uploaded: nothing was uploaded into this slot");
  SVO_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  SVO_HIP_CHECK(ctx, hipEventSynchronize(g->ev_up[slot]));  // started a whole batch ago in a streaming loop: long complete
  const int batch = g->up_batch[slot];
  g->up_batch[slot] = 0;
  const size_t lane_stride = (size_t)g->max_batch * (size_t)g->prm.width * (size_t)g->prm.height;
  return svo_pipeline_group_process_batch_dev(g, g->d_stage[slot][0], g->d_stage[slot][1], lane_stride, batch, results);
}

extern "C" int svo_pipeline_group_process_batch(svo_pipeline_group* g, const uint8_t* left, const uint8_t* right, size_t lane_stride,
                                                int batch, svo_frame_result* results) {
  if (!g) return SVO_ERR_INVALID;
  svo_ctx* ctx = g->ctx;
  SVO_REQUIRE(ctx, left && right && results && batch >= 1 && batch <= g->max_batch, "pipeline_group_process_batch: bad arguments");
  const size_t istride = (size_t)g->prm.width * (size_t)g->prm.height;
  SVO_REQUIRE(ctx, lane_stride >= istride * (size_t)batch, "pipeline_group_process_batch: lanes overlap");
  int rc = ensure_staging(g);
  if (rc) return rc;
  const size_t stage_stride = (size_t)g->max_batch * istride;
  for (int l = 0; l < g->n_lanes; ++l) {
    memcpy(g->h_stage[0][0] + (size_t)l * stage_stride, left + (size_t)l * lane_stride, (size_t)batch * istride);
    memcpy(g->h_stage[0][1] + (size_t)l * stage_stride, right + (size_t)l * lane_stride, (size_t)batch * istride);
  }
  if ((rc = svo_pipeline_group_upload(g, 0, batch))) return rc;
  return svo_pipeline_group_process_uploaded(g, 0, results);
}
