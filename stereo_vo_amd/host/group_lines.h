// The line policy of a pipeline group (host/group.cpp), free of the GPU: which queued lanes ride which line (stream) of a
// stage, whether a line's launch is ripe under the gather rule, and the order in which assembled solves are offered to the
// admission.  Pure functions of small arrays, plain ints and doubles: tests/sanitize/group_lines_test.cpp walks them on a CPU.
#ifndef SVO_GROUP_LINES_H_
#define SVO_GROUP_LINES_H_
#include <vector>

// a lane always rides the same line of a stage: stream order keeps its consecutive stages coherent
inline bool svo_line_carries(int lane, int line, int n_lines) { return lane % n_lines == line; }

// the lanes of `q` that ride line `line` of `n_lines`, in queue order, removed from q
inline std::vector<int> svo_line_take(std::vector<int>& q, int line, int n_lines) {
  std::vector<int> mine;
  for (size_t k = 0; k < q.size();) {
    if (svo_line_carries(q[k], line, n_lines)) { mine.push_back(q[k]); q.erase(q.begin() + (long)k); } else ++k;
  }
  return mine;
}

// GATHER (gather_us > 0): a launch lasts as long as its slowest item whatever it carries, so a bus that leaves with four of the
// line's lanes while others are a hundred microseconds away costs a whole launch more.  A stage's launch therefore waits while a
// lane of its line is NEAR (in the launch in flight of the stage before it, not queued), at most gather_us per waiting lane.
// queued_since(lane): when the lane entered q (microseconds, the clock of now_us); near(lane): over all n_lanes lanes.
template <typename QueuedSince, typename Near>
inline bool svo_line_ripe(const std::vector<int>& q, int n_lanes, int line, int n_lines, double now_us, double gather_us,
                          QueuedSince queued_since, Near near) {
  if (gather_us <= 0.0) return true;
  int mine = 0;
  bool waited = false;
  for (int li : q) if (svo_line_carries(li, line, n_lines)) { ++mine; waited = waited || now_us - queued_since(li) >= gather_us; }
  if (!mine || waited) return true;
  for (int li = 0; li < n_lanes; ++li) if (svo_line_carries(li, line, n_lines) && near(li)) return false;
  return true;
}

// Who is offered to the admission first (it may run out of budget behind any of them): a lane whose next keyframe already waits
// for this solve, then the solve that has waited longest (lowest ready_seq) — in lane order the high lanes of a large group
// starved and became the stragglers of the call (profiles/r04_group_sweep.txt: 56 and 64 lanes).
inline bool svo_solve_before(bool a_waits, unsigned long long a_ready_seq, bool b_waits, unsigned long long b_ready_seq) {
  if (a_waits != b_waits) return a_waits;
  return a_ready_seq < b_ready_seq;
}
// ... with solves that stepped aside after their LM iterations per launch (they keep the ready_seq of their first offer): behind the
// lanes whose keyframe waits, in front of the solves that have never run — what is half done is finished first, so that a solve's
// latency grows by the launches it needs and not by the queue behind it; first come, first served within each class.
inline bool svo_solve_before(bool a_waits, bool a_yielded, unsigned long long a_ready_seq, bool b_waits, bool b_yielded, unsigned long long b_ready_seq) {
  if (a_waits != b_waits) return a_waits;
  if (a_yielded != b_yielded) return a_yielded;
  return a_ready_seq < b_ready_seq;
}
#endif
