// The line policy of a pipeline group (stereo_vo_amd/host/group_lines.h) walked on the host, under ASan + UBSan:
//   * partition: for 1..8 lines and 0..64 queued lanes, the lines partition the queue — every lane on exactly one line, in
//     queue order, and what a line leaves behind keeps its order;
//   * gather off: gather_us = 0 is always ripe;
//   * gather on: a line is held back in exactly one case — it has a queued lane, none of its queued lanes has waited
//     gather_us, and a lane of that line is in the near state and not queued;
//   * solve order: a strict weak ordering (64 entries with ties are sorted by it), a waiting lane never behind a non-waiting one.
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "group_lines.h"

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { ++fails; fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

static unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
static unsigned rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (unsigned)(rng_state >> 32); }

static const int LANES = 64;

// `nq` distinct lanes of 0..63 in a random queue order
static std::vector<int> random_queue(int nq) {
  std::vector<int> all(LANES);
  for (int i = 0; i < LANES; ++i) all[i] = i;
  for (int i = LANES - 1; i > 0; --i) std::swap(all[i], all[rnd() % (unsigned)(i + 1)]);
  all.resize((size_t)nq);
  return all;
}

static void partition_case(int n_lines, int nq) {
  const std::vector<int> q0 = random_queue(nq);
  std::vector<int> q = q0, on_line(LANES, -1);
  for (int line = 0; line < n_lines; ++line) {
    std::vector<int> rest_expected;
    for (int li : q) if (li % n_lines != line) rest_expected.push_back(li);
    const std::vector<int> mine = svo_line_take(q, line, n_lines);
    CHECK(q == rest_expected, "%d lines, %d queued: line %d disturbed the lanes it left behind", n_lines, nq, line);
    size_t at = 0;  // mine is a subsequence of the queue: queue order
    for (int li : mine) {
      CHECK(li >= 0 && li < LANES && svo_line_carries(li, line, n_lines), "%d lines: lane %d on line %d", n_lines, li, line);
      CHECK(on_line[li] < 0, "%d lines: lane %d on lines %d and %d", n_lines, li, on_line[li], line);
      on_line[li] = line;
      while (at < q0.size() && q0[at] != li) ++at;
      CHECK(at < q0.size(), "%d lines, %d queued: line %d carries lane %d out of queue order", n_lines, nq, line, li);
      ++at;
    }
  }
  CHECK(q.empty(), "%d lines, %d queued: %zu lanes ride no line", n_lines, nq, q.size());
  for (int li : q0) CHECK(on_line[li] == li % n_lines, "%d lines: lane %d rides line %d", n_lines, li, on_line[li]);
}

enum { FAR = 0, NEAR = 1 };
struct Lanes { int state[LANES]; bool queued[LANES]; double t_q[LANES]; };

static bool ripe(const Lanes& L, const std::vector<int>& q, int line, int n_lines, double now, double gather_us) {
  return svo_line_ripe(q, LANES, line, n_lines, now, gather_us, [&](int li) { return L.t_q[li]; },
                       [&](int li) { return L.state[li] == NEAR && !L.queued[li]; });
}

static void gather_case(int n_lines, int nq, double gather_us) {
  const double now = 1000.0;
  Lanes L;
  const std::vector<int> q = random_queue(nq);
  for (int i = 0; i < LANES; ++i) { L.state[i] = rnd() % 4 == 0 ? NEAR : FAR; L.queued[i] = false; L.t_q[i] = 0.0; }
  for (int li : q) {
    L.queued[li] = true;
    const unsigned r = rnd() % 8;  // mostly fresh; sometimes exactly gather_us old (ripe: >=), sometimes older
    L.t_q[li] = r == 0 ? now - gather_us : (r == 1 ? now - 2.0 * gather_us : now - gather_us * (double)(rnd() % 1000) / 1001.0);
  }
  for (int line = 0; line < n_lines; ++line) {
    CHECK(ripe(L, q, line, n_lines, now, 0.0), "gather off: line %d of %d held back", line, n_lines);
    bool has_queued = false, one_waited = false, one_near = false;
    for (int li : q) if (li % n_lines == line) { has_queued = true; one_waited = one_waited || now - L.t_q[li] >= gather_us; }
    for (int li = 0; li < LANES; ++li) one_near = one_near || (li % n_lines == line && L.state[li] == NEAR && !L.queued[li]);
    const bool held = has_queued && !one_waited && one_near;
    CHECK(ripe(L, q, line, n_lines, now, gather_us) == !held, "gather %.0f us: line %d of %d, %d queued: expected %s (queued %d, waited %d, near %d)",
          gather_us, line, n_lines, nq, held ? "held" : "ripe", (int)has_queued, (int)one_waited, (int)one_near);
  }
}

struct Solve { bool waits; unsigned long long seq; };
static bool before(const Solve& a, const Solve& b) { return svo_solve_before(a.waits, a.seq, b.waits, b.seq); }
static bool same(const Solve& a, const Solve& b) { return !before(a, b) && !before(b, a); }

static void solve_order_case() {
  std::vector<Solve> s(64);
  for (Solve& x : s) { x.waits = rnd() % 3 == 0; x.seq = 1 + rnd() % 12; }  // 64 entries over 24 classes: ties
  const size_t n = s.size();
  for (size_t a = 0; a < n; ++a) {
    CHECK(!before(s[a], s[a]), "not irreflexive at %zu", a);
    for (size_t b = 0; b < n; ++b) {
      CHECK(!(before(s[a], s[b]) && before(s[b], s[a])), "not asymmetric at %zu, %zu", a, b);
      for (size_t c = 0; c < n; ++c) {
        CHECK(!(before(s[a], s[b]) && before(s[b], s[c])) || before(s[a], s[c]), "not transitive at %zu, %zu, %zu", a, b, c);
        CHECK(!(same(s[a], s[b]) && same(s[b], s[c])) || same(s[a], s[c]), "equivalence not transitive at %zu, %zu, %zu", a, b, c);
      }
    }
  }
  std::sort(s.begin(), s.end(), before);
  for (size_t i = 1; i < n; ++i) {
    CHECK(!before(s[i], s[i - 1]), "not sorted at %zu", i);
    CHECK(!(s[i].waits && !s[i - 1].waits), "a waiting lane behind a non-waiting one at %zu", i);
    CHECK(s[i].waits != s[i - 1].waits || s[i - 1].seq <= s[i].seq, "a later solve in front of an earlier one at %zu", i);
  }
}

int main() {
  for (int n_lines = 1; n_lines <= 8; ++n_lines)
    for (int nq = 0; nq <= LANES; ++nq) {
      partition_case(n_lines, nq);
      for (int rep = 0; rep < 4; ++rep) gather_case(n_lines, nq, rep % 2 ? 200.0 : 50.0);
    }
  for (int rep = 0; rep < 8; ++rep) solve_order_case();
  if (fails) { fprintf(stderr, "%d checks failed\n", fails); return 1; }
  printf("group lines ok\n");
  return 0;
}
