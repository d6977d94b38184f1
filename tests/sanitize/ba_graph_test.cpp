// The sliding-window graph of the bundle adjuster (stereo_vo_amd/host/ba_graph.h) walked on the host, under ASan + UBSan:
//   * ids are sequential across keyframes; new landmarks are truncated at max_features (at it, one past it, and to zero when the
//     tracked ones alone exceed it); the window pops its oldest pose at window_size + 1;
//   * an unknown tracked id is rejected with nothing committed;
//   * gather() against a sort-based restatement: ascending lists (K-way merge), one keyframe with a descending list (stable
//     sort), both paths on the same observations, equal ids in window-slot order, one id twice in one keyframe;
//   * write_back changes exactly the gathered landmarks and the K poses; the nothing-to-solve flag; reset.
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <tuple>
#include <vector>

#include "ba_graph.h"

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { ++fails; fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

struct Kf { double pose[7]; std::vector<int64_t> ids; std::vector<float> xy; };  // what the test itself knows of a keyframe in the window

static void set_pose(double* p, int tag) { for (int a = 0; a < 7; ++a) p[a] = 100.0 * tag + a; }
// pixels tell the observations apart whatever order a keyframe lists them in: by keyframe, id and how often the id came before
static float u_of(int kf, int64_t id, int earlier) { return (float)(1000 * kf + 8 * (int)id + earlier) + 0.25f; }

// A keyframe of tracked ids (in the given order) and n_new new landmarks; returns the status, appends to `mirror` on success.
static int add(BaGraph& g, std::vector<Kf>& mirror, int window_size, int tag, const std::vector<int64_t>& tracked, int n_new, int* kept,
               std::vector<int64_t>* new_ids_out = nullptr) {
  Kf kf;
  set_pose(kf.pose, tag);
  std::vector<float> txy(2 * tracked.size() + 1), nxy(2 * (size_t)n_new + 1), nxyz(3 * (size_t)n_new + 1);
  for (size_t i = 0; i < tracked.size(); ++i) {
    txy[2 * i] = u_of(tag, tracked[i], (int)std::count(tracked.begin(), tracked.begin() + (long)i, tracked[i])); txy[2 * i + 1] = -txy[2 * i];
  }
  for (int i = 0; i < n_new; ++i) {
    nxy[2 * i] = u_of(tag, 100 + i, 0); nxy[2 * i + 1] = -nxy[2 * i];
    for (int a = 0; a < 3; ++a) nxyz[3 * i + a] = (float)(tag + 0.001 * i + 10 * a);
  }
  std::vector<int64_t> new_ids((size_t)n_new + 1, -7);
  const char* err = nullptr;
  const int rc = g.add_keyframe(kf.pose, tracked.data(), txy.data(), (int)tracked.size(), nxy.data(), nxyz.data(), n_new, new_ids.data(), kept, &err);
  if (rc != SVO_OK) { CHECK(err != nullptr, "a refusal without a message"); return rc; }
  kf.ids = tracked;
  for (size_t i = 0; i < tracked.size(); ++i) { kf.xy.push_back(txy[2 * i]); kf.xy.push_back(txy[2 * i + 1]); }
  for (int i = 0; i < *kept; ++i) { kf.ids.push_back(new_ids[i]); kf.xy.push_back(nxy[2 * i]); kf.xy.push_back(nxy[2 * i + 1]); }
  CHECK(new_ids[*kept] == -7, "new_ids written past the kept landmarks");
  mirror.push_back(kf);
  if ((int)mirror.size() > window_size) mirror.erase(mirror.begin());
  if (new_ids_out) new_ids_out->assign(new_ids.begin(), new_ids.begin() + *kept);
  return rc;
}

static std::vector<float> points_of(const BaGraph& g, int n) {
  std::vector<int64_t> ids(n);
  for (int i = 0; i < n; ++i) ids[i] = i;
  std::vector<float> xyz(3 * (size_t)n + 1);
  const char* err = nullptr;
  CHECK(g.get_points(ids.data(), n, xyz.data(), &err) == SVO_OK, "get_points");
  return xyz;
}

// gather() against the restatement: every observation as (id, window slot, position in its keyframe), sorted.
static void check_gather(BaGraph& g, const std::vector<Kf>& mirror, const char* what) {
  std::vector<std::tuple<int64_t, int, int>> want;
  for (size_t k = 0; k < mirror.size(); ++k)
    for (size_t i = 0; i < mirror[k].ids.size(); ++i) want.emplace_back(mirror[k].ids[i], (int)k, (int)i);
  std::sort(want.begin(), want.end());
  const std::vector<float> world = points_of(g, g.feature_count());
  const BaProblemView v = g.gather();
  CHECK(v.K == (int)mirror.size() && v.M == (int)want.size(), "%s: K %d, M %d", what, v.K, v.M);
  if (v.K != (int)mirror.size() || v.M != (int)want.size()) return;
  for (int k = 0; k < v.K; ++k) CHECK(!memcmp(v.poses + 7 * k, mirror[k].pose, sizeof(double) * 7), "%s: pose %d", what, k);
  int j = -1;
  for (int o = 0; o < v.M; ++o) {
    const int64_t id = std::get<0>(want[o]);
    const int k = std::get<1>(want[o]), i = std::get<2>(want[o]);
    if (o == 0 || id != std::get<0>(want[o - 1])) ++j;
    CHECK(v.op[o] == k && v.oj[o] == j, "%s: observation %d is (pose %d, landmark %d), expected (%d, %d)", what, o, v.op[o], v.oj[o], k, j);
    CHECK(j < v.n_points && v.lm_ids[j] == id, "%s: landmark %d", what, j);
    CHECK(v.uv[2 * o] == (double)mirror[k].xy[2 * i] && v.uv[2 * o + 1] == (double)mirror[k].xy[2 * i + 1], "%s: pixel of observation %d", what, o);
    for (int a = 0; a < 3 && j < v.n_points; ++a) CHECK((float)v.points[3 * j + a] == world[3 * id + a], "%s: landmark %d position", what, j);
  }
  CHECK(v.n_points == j + 1, "%s: %d landmarks, expected %d", what, v.n_points, j + 1);
}

static bool same_problem(const BaProblemView& a, const std::vector<int32_t>& op, const std::vector<int32_t>& oj, const std::vector<double>& uv, const std::vector<int64_t>& ids) {
  return a.M == (int)op.size() && a.n_points == (int)ids.size() && !memcmp(a.op, op.data(), 4 * op.size()) && !memcmp(a.oj, oj.data(), 4 * oj.size()) &&
         !memcmp(a.uv, uv.data(), 8 * uv.size()) && !memcmp(a.lm_ids, ids.data(), 8 * ids.size());
}

int main() {
  const char* err = nullptr;
  // ---- ids, truncation, window pop
  {
    const int W = 3, MAXF = 10;
    BaGraph g;
    std::vector<Kf> m;
    g.init(W, MAXF);
    CHECK(g.window_count() == 0 && g.feature_count() == 0 && !g.new_frame_added(), "a fresh graph");
    int kept = -1;
    std::vector<int64_t> ids;
    CHECK(add(g, m, W, 0, {}, 4, &kept, &ids) == SVO_OK && kept == 4, "first keyframe");
    CHECK(ids == (std::vector<int64_t>{0, 1, 2, 3}) && g.new_frame_added(), "ids start at 0");
    CHECK(add(g, m, W, 1, {1, 3}, 8, &kept, &ids) == SVO_OK && kept == 8, "n_tracked + n_new = max_features keeps all");  // 2 + 8 = 10
    CHECK(ids.front() == 4 && ids.back() == 11 && g.feature_count() == 12, "ids go on where the last keyframe stopped");
    CHECK(add(g, m, W, 2, {0, 5}, 9, &kept, &ids) == SVO_OK && kept == 8, "one past max_features drops one");         // 2 + 9 = 11
    CHECK(ids.front() == 12 && ids.back() == 19 && g.feature_count() == 20 && g.window_count() == 3, "window at its size");
    std::vector<int64_t> many;
    for (int i = 0; i < MAXF + 1; ++i) many.push_back(i);
    CHECK(add(g, m, W, 3, many, 5, &kept, &ids) == SVO_OK && kept == 0 && g.feature_count() == 20, "n_tracked > max_features adds nothing");
    CHECK(g.window_count() == W, "the window pops at window_size + 1");
    double p[7], q[7];
    set_pose(q, 1);
    CHECK(g.get_pose(0, p, &err) == SVO_OK && !memcmp(p, q, sizeof(p)), "the oldest pose is gone: slot 0 is keyframe 1");
    set_pose(q, 3);
    CHECK(g.get_pose(-1, p, &err) == SVO_OK && !memcmp(p, q, sizeof(p)), "slot -1 is the newest");
    CHECK(g.get_pose(W, p, &err) == SVO_ERR_INVALID && g.get_pose(-W - 1, p, &err) == SVO_ERR_INVALID, "slots out of range");
    // unknown tracked ids: nothing committed
    for (int64_t bad : {(int64_t)20, (int64_t)-1}) {
      err = nullptr;
      CHECK(add(g, m, W, 4, {2, bad}, 3, &kept) == SVO_ERR_INVALID, "unknown id %lld accepted", (long long)bad);
      CHECK(g.window_count() == W && g.feature_count() == 20, "a rejected keyframe changed the graph");
      CHECK(g.get_pose(-1, p, &err) == SVO_OK && !memcmp(p, q, sizeof(p)), "a rejected keyframe changed the window");
    }
    CHECK(add(g, m, W, 4, {19}, 0, &kept) == SVO_OK && kept == 0, "the last known id is known");
    float xyz[3];
    int64_t id = 20;
    CHECK(g.get_points(&id, 1, xyz, &err) == SVO_ERR_INVALID, "get_points of an unknown id");
    id = 4;  // the first new landmark of keyframe 1
    CHECK(g.get_points(&id, 1, xyz, &err) == SVO_OK && xyz[0] == 1.0f && xyz[1] == 11.0f && xyz[2] == 21.0f, "get_points");
    check_gather(g, m, "merge path after truncations");
  }
  // ---- gather: merge path, sort path, both on the same observations
  {
    const int W = 5;
    BaGraph asc, desc;
    std::vector<Kf> ma, md;
    asc.init(W, 400); desc.init(W, 400);
    int kept;
    for (BaGraph* g : {&asc, &desc}) {
      std::vector<Kf>& m = g == &asc ? ma : md;
      add(*g, m, W, 0, {}, 6, &kept);                                  // ids 0..5
      add(*g, m, W, 1, {0, 2, 3, 5}, 3, &kept);                        // + 6..8
      if (g == &asc) add(*g, m, W, 2, {0, 1, 3, 6, 8}, 2, &kept);      // + 9, 10
      else add(*g, m, W, 2, {8, 6, 3, 1, 0}, 2, &kept);                // the same observations, tracked part descending
      add(*g, m, W, 3, {3, 3, 9}, 0, &kept);                           // one id twice in one keyframe (ascending: <=)
      add(*g, m, W, 4, {}, 1, &kept);                                  // a landmark seen once; landmarks 4, 7 seen by old keyframes only
    }
    check_gather(asc, ma, "ascending lists");
    const BaProblemView a = asc.gather();
    const std::vector<int32_t> op(a.op, a.op + a.M), oj(a.oj, a.oj + a.M);
    const std::vector<double> uv(a.uv, a.uv + 2 * a.M);
    const std::vector<int64_t> ids(a.lm_ids, a.lm_ids + a.n_points);
    // id 3: slots 0, 1, 2, then twice slot 3, in that order
    std::vector<int> slots3;
    for (int o = 0; o < a.M; ++o) if (a.lm_ids[a.oj[o]] == 3) slots3.push_back(a.op[o]);
    CHECK(slots3 == (std::vector<int>{0, 1, 2, 3, 3}), "an id of several keyframes comes out in window-slot order");
    const BaProblemView d = desc.gather();
    CHECK(same_problem(d, op, oj, uv, ids), "merge and stable sort disagree on the same observations");
    check_gather(desc, md, "one descending list");
    CHECK(same_problem(asc.gather(), op, oj, uv, ids), "gather twice");
  }
  // ---- write_back, the nothing-to-solve flag, reset
  {
    const int W = 2;
    BaGraph g;
    std::vector<Kf> m;
    g.init(W, 400);
    int kept;
    add(g, m, W, 0, {}, 5, &kept);
    add(g, m, W, 1, {1, 2}, 2, &kept);
    add(g, m, W, 2, {2, 5}, 1, &kept);  // window: keyframes 1, 2; gathered landmarks 1, 2, 5, 6, 7 — 0, 3, 4 are not
    CHECK(g.new_frame_added(), "a keyframe was added");
    const std::vector<float> before = points_of(g, g.feature_count());
    const BaProblemView v = g.gather();
    CHECK(v.K == 2 && v.n_points == 5, "gathered %d poses, %d landmarks", v.K, v.n_points);
    double* poses = g.solved_poses();
    double* pts = g.solved_points();
    for (int i = 0; i < 7 * v.K; ++i) poses[i] = -1.0 - i;
    for (int i = 0; i < 3 * v.n_points; ++i) pts[i] = 5000.0 + i;
    g.write_back(poses, pts);
    CHECK(!g.new_frame_added(), "write_back clears the flag");
    const std::vector<float> after = points_of(g, g.feature_count());
    const int64_t gathered[5] = {1, 2, 5, 6, 7};
    for (int id = 0; id < g.feature_count(); ++id) {
      const int64_t* at = std::find(gathered, gathered + 5, (int64_t)id);
      for (int a = 0; a < 3; ++a) {
        if (at == gathered + 5) CHECK(after[3 * id + a] == before[3 * id + a], "landmark %d was not gathered and changed", id);
        else CHECK(after[3 * id + a] == (float)(5000.0 + 3 * (at - gathered) + a), "landmark %d was gathered and kept %g", id, after[3 * id + a]);
      }
    }
    for (int k = 0; k < 2; ++k) {
      double p[7];
      CHECK(g.get_pose(k, p, &err) == SVO_OK, "get_pose");
      for (int a = 0; a < 7; ++a) CHECK(p[a] == -1.0 - (7 * k + a), "pose %d after write_back", k);
    }
    CHECK(g.window_count() == 2 && g.feature_count() == 8, "write_back changed the graph's shape");
    g.reset();
    CHECK(g.window_count() == 0 && g.feature_count() == 0 && !g.new_frame_added(), "reset");
    const BaProblemView e = g.gather();
    CHECK(e.K == 0 && e.M == 0 && e.n_points == 0, "an empty graph gathers nothing");
    m.clear();
    std::vector<int64_t> ids;
    CHECK(add(g, m, W, 7, {}, 2, &kept, &ids) == SVO_OK && ids == (std::vector<int64_t>{0, 1}), "ids restart after reset");
    CHECK(add(g, m, W, 8, {2}, 0, &kept) == SVO_ERR_INVALID, "ids of before the reset are unknown");
    check_gather(g, m, "after reset");
  }
  if (fails) { fprintf(stderr, "%d check(s) failed\n", fails); return 1; }
  printf("ba graph ok\n");
  return 0;
}
