// a9/a10/a13 — the sliding-window graph of the bundle adjuster (BundleAdjuster state, reference src/bundle_adjuster.cpp:41-135,
// 159-163; ids sequential — SURVEY C-3), free of the GPU: keyframes in, the window's observations out as a landmark-major
// problem, the solved poses and landmarks back in.  csrc/ba.hip wraps it in the C ABI; tests/sanitize/ba_graph_test.cpp walks it
// on a CPU.  Every scratch vector is a member: a keyframe's solve allocates nothing in steady state.
#ifndef SVO_BA_GRAPH_H_
#define SVO_BA_GRAPH_H_
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <deque>
#include <vector>

#include "svo.h"

// What gather() hands to the solver: K poses (slot 0 the oldest), the landmarks some pose of the window observes in ascending id
// order, the observations sorted by (landmark, window slot).  Valid until the next gather().
struct BaProblemView {
  int K; const double* poses;             // 7 per pose
  int n_points; const double* points;     // 3 per landmark
  int M; const int32_t *op, *oj; const double* uv;  // per observation: window slot, landmark index, pixel (2)
  const int64_t* lm_ids;                  // per landmark: its feature id
};

class BaGraph {
 public:
  void init(int window_size, int max_features) { window_size_ = window_size; max_features_ = max_features; }
  int window_count() const { return (int)window_.size(); }
  int feature_count() const { return (int)(feat_pos_.size() / 3); }
  bool new_frame_added() const { return new_frame_added_; }  // false: nothing to solve (src/bundle_adjuster.cpp:138)

  // Returns SVO_OK, or SVO_ERR_INVALID with *err set and nothing committed.
  int add_keyframe(const double* pose7, const int64_t* tracked_ids, const float* tracked_xy, int n_tracked, const float* new_xy,
                   const float* new_xyz, int n_new, int64_t* new_ids, int* n_new_out, const char** err) {
    PoseVar pv;
    memcpy(pv.pose, pose7, sizeof(pv.pose));  // src/bundle_adjuster.cpp:63-70
    const int64_t nfeat = feature_count();
    for (int i = 0; i < n_tracked; ++i) {   // :72-83
      if (!(tracked_ids[i] >= 0 && tracked_ids[i] < nfeat)) { *err = "ba_add_keyframe: unknown feature id"; return SVO_ERR_INVALID; }
      pv.obs.push_back({tracked_xy[2 * i], tracked_xy[2 * i + 1], tracked_ids[i]});
    }
    const int max_new = n_tracked > max_features_ ? 0 : max_features_ - n_tracked;  // :85-90 with the C-5 guard
    const int keep = n_new > max_new ? max_new : n_new;
    for (int i = 0; i < keep; ++i) {        // :92-122; ids sequential (C-3), new_ids = real ids only (C-4)
      const int64_t id = feature_count();
      feat_pos_.insert(feat_pos_.end(), new_xyz + 3 * i, new_xyz + 3 * i + 3);
      new_ids[i] = id;
      pv.obs.push_back({new_xy[2 * i], new_xy[2 * i + 1], id});
    }
    *n_new_out = keep;
    window_.push_back(std::move(pv));
    if ((int)window_.size() > window_size_) window_.pop_front();  // :126-128 (remove_oldest_pose)
    new_frame_added_ = true;                                      // :134
    return SVO_OK;
  }

  void reset() { window_.clear(); feat_pos_.clear(); new_frame_added_ = false; lm_ids_.clear(); s_poses_.clear(); }  // (a gathered problem goes with its graph)

  int get_pose(int k, double* pose7, const char** err) const {
    const int K = window_count();
    if (k < 0) k += K;
    if (!(k >= 0 && k < K)) { *err = "ba_get_pose: slot out of range"; return SVO_ERR_INVALID; }
    memcpy(pose7, window_[k].pose, 7 * sizeof(double));
    return SVO_OK;
  }

  int get_points(const int64_t* ids, int n, float* xyz, const char** err) const {
    const int64_t nfeat = feature_count();
    for (int i = 0; i < n; ++i) {  // src/bundle_adjuster.cpp:159-163 (double -> float)
      if (!(ids[i] >= 0 && ids[i] < nfeat)) { *err = "ba_get_points: unknown feature id"; return SVO_ERR_INVALID; }
      for (int a = 0; a < 3; ++a) xyz[3 * i + a] = (float)feat_pos_[3 * ids[i] + a];
    }
    return SVO_OK;
  }

  // Observations sorted by (landmark id, window slot) — the order ceres would visit nothing in particular, but the
  // declared summation order is defined on it.  Every keyframe's observation list is ascending in id when it comes
  // from the pipeline (tracked ids keep their order, new ids are larger), so a K-way merge replaces the sort; lists
  // from other callers are checked and fall back to a stable sort.
  BaProblemView gather() {
    const int K = window_count();
    s_poses_.resize(7 * (size_t)K); s_points_.clear(); s_uv_.clear(); s_op_.clear(); s_oj_.clear(); lm_ids_.clear();
    s_points_.reserve(3 * 4096); s_uv_.reserve(2 * 4096); s_op_.reserve(4096); s_oj_.reserve(4096); lm_ids_.reserve(4096);
    for (int k = 0; k < K; ++k) memcpy(&s_poses_[7 * k], window_[k].pose, 7 * sizeof(double));
    bool ascending = true;
    size_t total = 0;
    for (int k = 0; k < K; ++k) {
      const auto& o = window_[k].obs;
      total += o.size();
      for (size_t i = 1; i < o.size() && ascending; ++i) ascending = o[i - 1].id <= o[i].id;
    }
    auto emit = [&](int k, const Obs& o) {
      if (lm_ids_.empty() || lm_ids_.back() != o.id) {
        lm_ids_.push_back(o.id);
        for (int a = 0; a < 3; ++a) s_points_.push_back(feat_pos_[3 * o.id + a]);
      }
      s_op_.push_back(k); s_oj_.push_back((int32_t)lm_ids_.size() - 1);
      s_uv_.push_back(o.u); s_uv_.push_back(o.v);
    };
    if (ascending && K <= 64) {
      const Obs* cur[64];
      const Obs* end[64];
      for (int k = 0; k < K; ++k) { const auto& o = window_[k].obs; cur[k] = o.data(); end[k] = o.data() + o.size(); }
      for (size_t done = 0; done < total; ++done) {
        int best = -1;
        int64_t best_id = 0;
        for (int k = 0; k < K; ++k)  // smallest id first; equal ids in window-slot order (what the stable sort gives)
          if (cur[k] != end[k] && (best < 0 || cur[k]->id < best_id)) { best = k; best_id = cur[k]->id; }
        emit(best, *cur[best]++);
      }
    } else {
      struct Flat { int k; const Obs* o; };
      std::vector<Flat> flat;
      flat.reserve(total);
      for (int k = 0; k < K; ++k)
        for (const auto& o : window_[k].obs) flat.push_back({k, &o});
      std::stable_sort(flat.begin(), flat.end(), [](const Flat& a, const Flat& b) { return a.o->id < b.o->id; });
      for (const Flat& f : flat) emit(f.k, *f.o);
    }
    return {K, s_poses_.data(), (int)lm_ids_.size(), s_points_.data(), (int)s_op_.size(), s_op_.data(), s_oj_.data(), s_uv_.data(), lm_ids_.data()};
  }

  // Where the solver may leave the gathered problem's solved poses (7 K) and landmarks (3 n_points) for write_back.
  double* solved_poses() { return s_poses_.data(); }
  double* solved_points() { s_out_pts_.resize(s_points_.size()); return s_out_pts_.data(); }
  const std::vector<int64_t>& gathered_ids() const { return lm_ids_; }

  // The solved poses of the gathered window slots and the solved gathered landmarks into the graph (src/bundle_adjuster.cpp:146-155).
  void write_back(const double* poses7, const double* points3) {
    const size_t K = s_poses_.size() / 7;
    for (size_t k = 0; k < K; ++k) memcpy(window_[k].pose, &poses7[7 * k], 7 * sizeof(double));
    for (size_t l = 0; l < lm_ids_.size(); ++l)
      for (int a = 0; a < 3; ++a) feat_pos_[3 * lm_ids_[l] + a] = points3[3 * l + a];
    new_frame_added_ = false;  // :155
  }

 private:
  struct Obs { float u, v; int64_t id; };
  struct PoseVar { double pose[7]; std::vector<Obs> obs; };
  int window_size_ = 5, max_features_ = 0;
  std::deque<PoseVar> window_;
  std::vector<double> feat_pos_;  // 3 per feature id
  bool new_frame_added_ = false;
  std::vector<int64_t> lm_ids_;   // the gathered landmarks' feature ids
  std::vector<double> s_poses_, s_points_, s_uv_, s_out_pts_;  // gather scratch
  std::vector<int32_t> s_op_, s_oj_;
};

#endif
