// The order in which a pipeline group offers its assembled solves to the admission (host/group_lines.h: svo_solve_before with solves
// that stepped aside), walked on a CPU under ASan + UBSan: the comparator sorts random queues the way host/group.cpp's does, and the
// result is checked against the three rules — a lane whose keyframe waits comes first; among the waiting lanes and among the others a
// solve that has run before comes before a fresh one; first come, first served within each of the four classes.
#include <algorithm>
#include <cstdio>
#include <random>
#include <vector>

#include "group_lines.h"

struct Solve { bool waits, yielded; unsigned long long seq; };

static bool before(const Solve& a, const Solve& b) { return svo_solve_before(a.waits, a.yielded, a.seq, b.waits, b.yielded, b.seq); }
static int cls(const Solve& s) { return (s.waits ? 0 : 2) + (s.yielded ? 0 : 1); }  // four classes: waiting lanes first, and within either half what has run before

int main() {
  std::mt19937 rng(0x5EED09u);
  long checked = 0;
  for (int round = 0; round < 2000; ++round) {
    const int n = 1 + (int)(rng() % 64u);
    std::vector<Solve> q((size_t)n);
    std::vector<unsigned long long> seqs((size_t)n);
    for (int i = 0; i < n; ++i) seqs[(size_t)i] = 1ull + (unsigned long long)i + 1000ull * (unsigned long long)round;  // distinct, as ba_ready_counter hands them out
    std::shuffle(seqs.begin(), seqs.end(), rng);
    for (int i = 0; i < n; ++i) q[(size_t)i] = Solve{rng() % 4u == 0, rng() % 3u == 0, seqs[(size_t)i]};
    // a strict weak order: irreflexive, asymmetric
    for (const Solve& a : q) {
      if (before(a, a)) { fprintf(stderr, "not irreflexive\n"); return 1; }
      for (const Solve& b : q)
        if (before(a, b) && before(b, a)) { fprintf(stderr, "not asymmetric\n"); return 1; }
    }
    std::sort(q.begin(), q.end(), before);
    for (int i = 0; i + 1 < n; ++i) {
      const Solve &a = q[(size_t)i], &b = q[(size_t)i + 1];
      if (cls(a) > cls(b)) { fprintf(stderr, "class order broken at %d: %d before %d\n", i, cls(a), cls(b)); return 1; }
      if (cls(a) == cls(b) && !(a.seq < b.seq)) { fprintf(stderr, "not first come, first served within class %d\n", cls(a)); return 1; }
      ++checked;
    }
  }
  // the cases by name
  const Solve fresh_old{false, false, 1}, yielded_new{false, true, 9}, waits_fresh{true, false, 20}, waits_yielded{true, true, 30};
  if (!before(yielded_new, fresh_old) || before(fresh_old, yielded_new)) { fprintf(stderr, "a solve that stepped aside must come before a fresh one\n"); return 1; }
  if (!before(waits_fresh, yielded_new) || !before(waits_fresh, fresh_old)) { fprintf(stderr, "a lane whose keyframe waits must come first\n"); return 1; }
  if (!before(waits_yielded, waits_fresh)) { fprintf(stderr, "among the lanes that wait: what has run before comes first\n"); return 1; }
  if (!before(waits_yielded, yielded_new)) { fprintf(stderr, "a lane whose keyframe waits must come first among the solves that stepped aside\n"); return 1; }
  // without solves that stepped aside the order is the one of the four-argument form
  for (unsigned m = 0; m < 4; ++m)
    if (svo_solve_before((m & 1u) != 0, false, 3, (m & 2u) != 0, false, 5) != svo_solve_before((m & 1u) != 0, 3, (m & 2u) != 0, 5)) { fprintf(stderr, "differs from the plain order\n"); return 1; }
  printf("solve order ok (%ld neighbours)\n", checked);
  return 0;
}
