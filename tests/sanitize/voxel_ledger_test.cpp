// The keyframe ledger's table (stereo_vo_amd/host/voxel_ledger.h) walked on the host, under ASan + UBSan:
//   * the pure byte count and every refusal of the parameters;
//   * fill, refuse when full, duplicate and unknown ids, oversize and negative n, with nothing changed by a refusal;
//   * retire / remove (one release) in every order of three held ids, and the reuse of the freed slots;
//   * the recorded pose and matrix being the inserted ones, and the moved ones after an update;
//   * 10,000 random operations against a std::map model: the held set, every record, and that no two ids share a slot.
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <random>
#include <set>
#include <vector>

#include "voxel_ledger.h"

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { ++fails; fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

struct Rec { int n; double pose[7]; double m[12]; int slot; };

static void fill(double* pose, double* m, int tag) {
  for (int a = 0; a < 7; ++a) pose[a] = 10.0 * tag + a + 0.125;
  for (int a = 0; a < 12; ++a) m[a] = -3.0 * tag + 0.5 * a;
}

// insert through admit + hold, as csrc does; returns the status
static int put(VoxelLedgerTable& t, int64_t id, int n, int tag, std::map<int64_t, Rec>* model, const char** err) {
  int slot = -1;
  const int rc = t.admit(id, n, &slot, err);
  if (rc != SVO_OK) return rc;
  Rec r;
  r.n = n; r.slot = slot;
  fill(r.pose, r.m, tag);
  t.hold(slot, id, n, r.pose, r.m);
  if (model) (*model)[id] = r;
  return rc;
}

static void same_as_model(const VoxelLedgerTable& t, const std::map<int64_t, Rec>& model, const char* where) {
  CHECK(t.held() == (int)model.size(), "%s: %d held, the model has %zu", where, t.held(), model.size());
  std::vector<int64_t> ids((size_t)t.max_keyframes() + 1, -99);
  int n = -1;
  const char* err = nullptr;
  CHECK(t.ids(ids.data(), t.max_keyframes(), &n, &err) == SVO_OK && n == (int)model.size(), "%s: ids", where);
  CHECK(ids[(size_t)t.max_keyframes()] == -99, "%s: ids written past the capacity", where);
  std::set<int> slots;
  int k = 0;
  for (const auto& e : model) {  // std::map: ascending, as ids() promises
    CHECK(k < n && ids[(size_t)k] == e.first, "%s: id %d", where, k);
    ++k;
    int slot = -1;
    CHECK(t.find(e.first, &slot, "unknown", &err) == SVO_OK, "%s: a held id is not found", where);
    if (slot < 0) continue;
    CHECK(slot == e.second.slot && slot < t.max_keyframes(), "%s: slot", where);
    CHECK(slots.insert(slot).second, "%s: two ids share slot %d", where, slot);
    const VoxelLedgerSlot& s = t.slot(slot);
    CHECK(s.held && s.id == e.first && s.n == e.second.n, "%s: record", where);
    CHECK(memcmp(s.pose7, e.second.pose, sizeof(s.pose7)) == 0 && memcmp(s.m12, e.second.m, sizeof(s.m12)) == 0, "%s: pose or matrix bits", where);
  }
}

int main() {
  const char* err = nullptr;
  // ---- the byte count and the parameters
  {
    size_t b = 7;
    svo_voxel_ledger_params p = {4, 1000};
    CHECK(VoxelLedgerTable::bytes(&p, &b) == SVO_OK && b == (size_t)16 * 4 * 1000, "bytes");
    p = {1, 1};
    CHECK(VoxelLedgerTable::bytes(&p, &b) == SVO_OK && b == 16, "bytes of the smallest ledger");
    p = {65536, 1 << 20};
    CHECK(VoxelLedgerTable::bytes(&p, &b) == SVO_OK && b == (size_t)1 << 40, "bytes of a large ledger");
    p = {2147483647, 2147483647};  // 16 * (2^31 - 1)^2 is beyond 2^64
    b = 7;
    CHECK(VoxelLedgerTable::bytes(&p, &b) == SVO_ERR_INVALID && b == 0, "a product beyond size_t is refused");
    p = {4, 1000};
    const svo_voxel_ledger_params bad[] = {{0, 5}, {-1, 5}, {5, 0}, {5, -3}};
    for (const auto& q : bad) {
      b = 7;
      CHECK(VoxelLedgerTable::bytes(&q, &b) == SVO_ERR_INVALID && b == 0, "bytes of refused parameters");
      VoxelLedgerTable t;
      err = nullptr;
      CHECK(t.init(&q, &err) == SVO_ERR_INVALID && err && strstr(err, q.max_keyframes < 1 ? "max_keyframes" : "max_points"), "init refuses and names the field");
    }
    b = 7;
    CHECK(VoxelLedgerTable::bytes(nullptr, &b) == SVO_ERR_INVALID && b == 0, "null params");
    CHECK(VoxelLedgerTable::bytes(&p, nullptr) == SVO_ERR_INVALID, "null bytes");
    VoxelLedgerTable t;
    CHECK(t.init(nullptr, &err) == SVO_ERR_INVALID && strstr(err, "params"), "init: null params");
  }
  // ---- fill, full, duplicate, unknown, oversize
  {
    VoxelLedgerTable t;
    const svo_voxel_ledger_params p = {3, 100};
    CHECK(t.init(&p, &err) == SVO_OK && t.held() == 0 && t.max_keyframes() == 3 && t.max_points() == 100, "init");
    std::map<int64_t, Rec> model;
    CHECK(put(t, 7, 100, 1, &model, &err) == SVO_OK && model[7].slot == 0, "the first insert takes slot 0");
    CHECK(put(t, 7, 10, 2, nullptr, &err) == SVO_ERR_INVALID && strstr(err, "already held"), "a duplicate id is refused");
    CHECK(put(t, 8, 101, 2, nullptr, &err) == SVO_ERR_INVALID && strstr(err, "max_points"), "n beyond max_points is refused");
    CHECK(put(t, 8, -1, 2, nullptr, &err) == SVO_ERR_INVALID && strstr(err, "negative"), "a negative n is refused");
    same_as_model(t, model, "after the refusals");
    CHECK(put(t, -5, 0, 2, &model, &err) == SVO_OK, "a negative id and an empty cloud are fine");
    CHECK(put(t, (int64_t)1 << 40, 1, 3, &model, &err) == SVO_OK, "a large id");
    CHECK(put(t, 9, 1, 4, nullptr, &err) == SVO_ERR_INVALID && strstr(err, "no free slot"), "a full ledger refuses");
    same_as_model(t, model, "full");
    int slot = -1;
    CHECK(t.find(9, &slot, "voxel_ledger_update: unknown id", &err) == SVO_ERR_INVALID && !strcmp(err, "voxel_ledger_update: unknown id") && slot == -1,
          "an unknown id is refused with the caller's words");
    // the recorded matrix is the inserted one; an update replaces both
    CHECK(t.find(7, &slot, "unknown", &err) == SVO_OK, "find");
    Rec moved;
    fill(moved.pose, moved.m, 55);
    t.moved(slot, moved.pose, moved.m);
    memcpy(model[7].pose, moved.pose, sizeof(moved.pose));
    memcpy(model[7].m, moved.m, sizeof(moved.m));
    same_as_model(t, model, "after an update");
    // ids with a short buffer: the count is still the whole
    int64_t two[3] = {-99, -99, -99};
    int n = 0;
    CHECK(t.ids(two, 2, &n, &err) == SVO_OK && n == 3 && two[0] == -5 && two[1] == 7 && two[2] == -99, "ids into a short buffer");
    CHECK(t.ids(nullptr, 0, &n, &err) == SVO_OK && n == 3, "ids only counted");
    CHECK(t.ids(nullptr, 2, &n, &err) == SVO_ERR_INVALID && t.ids(two, -1, &n, &err) == SVO_ERR_INVALID && t.ids(two, 2, nullptr, &err) == SVO_ERR_INVALID,
          "ids: refusals");
  }
  // ---- release in every order of three, and reuse
  {
    int order[3] = {0, 1, 2};
    int perms = 0;
    do {
      ++perms;
      VoxelLedgerTable t;
      const svo_voxel_ledger_params p = {3, 8};
      CHECK(t.init(&p, &err) == SVO_OK, "init");
      std::map<int64_t, Rec> model;
      for (int i = 0; i < 3; ++i) CHECK(put(t, 100 + i, i + 1, i, &model, &err) == SVO_OK, "fill");
      for (int k = 0; k < 3; ++k) {
        const int64_t id = 100 + order[k];
        int slot = -1;
        CHECK(t.find(id, &slot, "unknown", &err) == SVO_OK, "find before the release");
        t.release(slot);
        model.erase(id);
        same_as_model(t, model, "after a release");
        CHECK(t.find(id, &slot, "unknown", &err) == SVO_ERR_INVALID, "a released id is unknown");
        // the freed slot is the next one handed out, and the others keep theirs
        CHECK(put(t, 200 + k, 2, 9, &model, &err) == SVO_OK && model[200 + k].slot == slot, "the freed slot is reused");
        same_as_model(t, model, "after the reuse");
        int s2 = -1;
        CHECK(t.find(200 + k, &s2, "unknown", &err) == SVO_OK, "find the new id");
        t.release(s2);
        model.erase(200 + k);
      }
      CHECK(t.held() == 0, "everything released");
      for (int i = 0; i < 3; ++i) CHECK(put(t, 300 + i, 1, i, &model, &err) == SVO_OK, "an emptied ledger fills again");
      CHECK(put(t, 999, 1, 0, nullptr, &err) == SVO_ERR_INVALID, "and is full again");
    } while (std::next_permutation(order, order + 3));
    CHECK(perms == 6, "six orders");
  }
  // ---- random operations against the model
  {
    VoxelLedgerTable t;
    const svo_voxel_ledger_params p = {6, 50};
    CHECK(t.init(&p, &err) == SVO_OK, "init");
    std::map<int64_t, Rec> model;
    std::mt19937 rng(12345);
    int n_put = 0, n_full = 0, n_dup = 0, n_rel = 0, n_unknown = 0, n_moved = 0, n_big = 0;
    for (int step = 0; step < 10000; ++step) {
      const int64_t id = (int64_t)(rng() % 12) - 3;
      const int op = (int)(rng() % 4);
      if (op == 0) {
        const int n = (int)(rng() % 56);  // 51..55 are beyond max_points
        const bool dup = model.count(id) != 0, full = model.size() == 6, big = n > 50;
        const int rc = put(t, id, n, step, &model, &err);
        CHECK((rc == SVO_OK) == !(dup || full || big), "step %d: insert", step);
        if (rc == SVO_OK) ++n_put; else if (big) ++n_big; else if (dup) ++n_dup; else ++n_full;
      } else {
        int slot = -1;
        const int rc = t.find(id, &slot, "unknown", &err);
        CHECK((rc == SVO_OK) == (model.count(id) != 0), "step %d: find", step);
        if (rc != SVO_OK) { ++n_unknown; continue; }
        if (op == 1) {
          Rec& r = model[id];
          fill(r.pose, r.m, -step);
          t.moved(slot, r.pose, r.m);
          ++n_moved;
        } else {  // retire and remove are one release
          t.release(slot);
          model.erase(id);
          ++n_rel;
        }
      }
      if (step % 16 == 0) same_as_model(t, model, "random walk");
    }
    same_as_model(t, model, "the end of the random walk");
    CHECK(n_put > 500 && n_full > 10 && n_dup > 100 && n_rel > 500 && n_unknown > 500 && n_moved > 500 && n_big > 50,
          "the walk reached every case: %d %d %d %d %d %d %d", n_put, n_full, n_dup, n_rel, n_unknown, n_moved, n_big);
  }
  if (fails) { fprintf(stderr, "%d failures\n", fails); return 1; }
  printf("voxel ledger ok\n");
  return 0;
}
