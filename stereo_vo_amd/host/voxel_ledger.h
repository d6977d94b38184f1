// The keyframe ledger of the voxel map (include/svo.h, "voxel map ledger"), free of the GPU: which keyframe id holds
// which slot of the device copy, how many records it has, and under which pose7 and camera->world matrix its cloud was last
// inserted (the later removal must use the very bits).  csrc/voxel.hip owns the device memory and the launches and asks this
// table before and after them; tests/sanitize/voxel_ledger_test.cpp walks it on a CPU.  The slot table and the free list are sized by
// init(); only the id -> slot map takes a host node per held id.
#ifndef SVO_VOXEL_LEDGER_H_
#define SVO_VOXEL_LEDGER_H_
#include <stdint.h>
#include <string.h>

#include <map>
#include <vector>

#include "svo.h"

struct VoxelLedgerSlot {
  int64_t id = 0;
  int n = 0;
  bool held = false;
  double pose7[7] = {0, 0, 0, 0, 0, 0, 0};
  double m12[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
};

class VoxelLedgerTable {
 public:
  // Pure: 16 bytes per record.  SVO_ERR_INVALID and *bytes = 0 for parameters init() refuses (or a product beyond size_t).
  static int bytes(const svo_voxel_ledger_params* p, size_t* out) {
    if (!out) return SVO_ERR_INVALID;
    *out = 0;
    if (!p || p->max_keyframes < 1 || p->max_points < 1) return SVO_ERR_INVALID;
    const unsigned long long k = (unsigned long long)p->max_keyframes, n = (unsigned long long)p->max_points;  // below 2^62 together
    if (k * n > (unsigned long long)(SIZE_MAX / 16)) return SVO_ERR_INVALID;
    *out = (size_t)(16ull * k * n);
    return SVO_OK;
  }

  int init(const svo_voxel_ledger_params* p, const char** err) {
    if (!p) { *err = "voxel_ledger_create: null params"; return SVO_ERR_INVALID; }
    if (p->max_keyframes < 1) { *err = "voxel_ledger_create: max_keyframes must be at least 1"; return SVO_ERR_INVALID; }
    if (p->max_points < 1) { *err = "voxel_ledger_create: max_points must be at least 1"; return SVO_ERR_INVALID; }
    size_t b;
    if (bytes(p, &b)) { *err = "voxel_ledger_create: max_keyframes * max_points is beyond the address space"; return SVO_ERR_INVALID; }
    max_keyframes_ = p->max_keyframes; max_points_ = p->max_points;
    slots_.assign((size_t)max_keyframes_, VoxelLedgerSlot());
    free_.clear();
    free_.reserve((size_t)max_keyframes_);
    for (int s = max_keyframes_ - 1; s >= 0; --s) free_.push_back(s);  // slot 0 is handed out first
    by_id_.clear();
    return SVO_OK;
  }

  int max_keyframes() const { return max_keyframes_; }
  int max_points() const { return max_points_; }
  int held() const { return (int)by_id_.size(); }
  const VoxelLedgerSlot& slot(int s) const { return slots_[(size_t)s]; }

  // May a cloud of n records come in under this id?  SVO_OK and the slot it would get, or SVO_ERR_INVALID with *err set.
  // Nothing changes: the caller commits with hold() once its copy and its insert are on the stream.
  int admit(int64_t id, int n, int* slot_out, const char** err) const {
    if (n < 0) { *err = "voxel_ledger_insert: n must not be negative"; return SVO_ERR_INVALID; }
    if (n > max_points_) { *err = "voxel_ledger_insert: n is beyond max_points"; return SVO_ERR_INVALID; }
    if (by_id_.count(id)) { *err = "voxel_ledger_insert: id is already held"; return SVO_ERR_INVALID; }
    if (free_.empty()) { *err = "voxel_ledger_insert: no free slot (max_keyframes are held)"; return SVO_ERR_INVALID; }
    *slot_out = free_.back();
    return SVO_OK;
  }

  // The slot admit() named now holds id: n records inserted under pose7, whose matrix was m12.
  void hold(int slot, int64_t id, int n, const double* pose7, const double* m12) {
    free_.pop_back();  // admit() named free_.back()
    VoxelLedgerSlot& s = slots_[(size_t)slot];
    s.id = id; s.n = n; s.held = true;
    memcpy(s.pose7, pose7, sizeof(s.pose7));
    memcpy(s.m12, m12, sizeof(s.m12));
    by_id_[id] = slot;
  }

  int find(int64_t id, int* slot_out, const char* what, const char** err) const {
    const auto it = by_id_.find(id);
    if (it == by_id_.end()) { *err = what; return SVO_ERR_INVALID; }
    *slot_out = it->second;
    return SVO_OK;
  }

  // The held cloud now sits in the map under this pose.
  void moved(int slot, const double* pose7, const double* m12) {
    VoxelLedgerSlot& s = slots_[(size_t)slot];
    memcpy(s.pose7, pose7, sizeof(s.pose7));
    memcpy(s.m12, m12, sizeof(s.m12));
  }

  // The slot is free for the next insert (retire and remove differ only in what the caller did to the map before).
  void release(int slot) {
    VoxelLedgerSlot& s = slots_[(size_t)slot];
    by_id_.erase(s.id);
    s.held = false; s.n = 0;
    free_.push_back(slot);
  }

  // The held ids in ascending order: at most `capacity` of them are written, *n is how many are held.
  int ids(int64_t* out, int capacity, int* n, const char** err) const {
    if (!n) { *err = "voxel_ledger_ids: null n"; return SVO_ERR_INVALID; }
    if (capacity < 0) { *err = "voxel_ledger_ids: capacity must not be negative"; return SVO_ERR_INVALID; }
    if (!out && capacity > 0) { *err = "voxel_ledger_ids: null ids"; return SVO_ERR_INVALID; }
    int k = 0;
    for (const auto& e : by_id_) {
      if (k < capacity) out[k] = e.first;
      ++k;
    }
    *n = k;
    return SVO_OK;
  }

 private:
  int max_keyframes_ = 0, max_points_ = 0;
  std::vector<VoxelLedgerSlot> slots_;
  std::vector<int> free_;            // a stack: the slot freed last is used first
  std::map<int64_t, int> by_id_;     // id -> slot
};

#endif  // SVO_VOXEL_LEDGER_H_
