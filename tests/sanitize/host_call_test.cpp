// The order rule of every synchronous entry and the layout of its temporary buffer (stereo_vo_amd/host/host_call.h) walked on the
// host, under ASan + UBSan, with a fake error type in place of HIP's:
//   * all 16 combinations of {the copies up fail, the _dev entry refuses, the copies back fail, the drain fails} against a restatement
//     written from the rule: which callables ran and in what order, the drain exactly once and last, the returned code, the error;
//   * SVO_ARGS_CHECK: a refusal's text goes into the context with SVO_ERR_INVALID, an acceptance changes nothing;
//   * the carver: offsets multiples of 256, parts disjoint and in order, zero-byte parts take no room, total() at least the sum of
//     the parts, sizes up to 2^40 without a wrap.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "host_call.h"
#include "svo.h"

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { ++fails; fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

// a fake error type: 0 is success, as Err() has to be
enum FakeErr { FAKE_OK = 0, FAKE_UP = 11, FAKE_BACK = 22, FAKE_DRAIN = 33, FAKE_UNSET = 99 };
constexpr int DEV_REFUSAL = -7;  // any non-zero code: it is handed on as it is

static void sequence() {
  for (int mask = 0; mask < 16; ++mask) {
    const bool up_fails = mask & 1, dev_refuses = mask & 2, back_fails = mask & 4, drain_fails = mask & 8;
    std::string ran;
    FakeErr failed = FAKE_UNSET;
    const int rc = svo_host_sequence(
        up_fails ? FAKE_UP : FAKE_OK, [&] { ran += 'd'; return dev_refuses ? DEV_REFUSAL : 0; },
        [&] { ran += 'b'; return back_fails ? FAKE_BACK : FAKE_OK; }, [&] { ran += 's'; return drain_fails ? FAKE_DRAIN : FAKE_OK; }, &failed);
    // the restatement: dev only after good copies up, back only after a dev that ran and returned 0, the drain once, always and last
    std::string want_ran;
    if (!up_fails) want_ran += 'd';
    const bool dev_ok = !up_fails && !dev_refuses;
    if (dev_ok) want_ran += 'b';
    want_ran += 's';
    // a refusal is returned as it is; otherwise the first failing of (up, back, drain)
    const int want_rc = !up_fails && dev_refuses ? DEV_REFUSAL : 0;
    const FakeErr want_failed = up_fails ? FAKE_UP : dev_ok && back_fails ? FAKE_BACK : drain_fails ? FAKE_DRAIN : FAKE_OK;
    CHECK(ran == want_ran, "mask %d: ran '%s', wanted '%s'", mask, ran.c_str(), want_ran.c_str());
    size_t drains = 0;
    for (char ch : ran) drains += ch == 's';
    CHECK(drains == 1 && !ran.empty() && ran.back() == 's', "mask %d: the drain ran %zu times in '%s'", mask, drains, ran.c_str());
    CHECK(rc == want_rc, "mask %d: returned %d, wanted %d", mask, rc, want_rc);
    if (!want_rc) CHECK(failed == want_failed, "mask %d: reported %d, wanted %d", mask, (int)failed, (int)want_failed);
    else CHECK(failed != FAKE_UNSET, "mask %d: the error was left unset", mask);
  }
}

struct FakeCtx { const char* err = nullptr; };
static int refuse_if(bool refuse, const char** err) {
  if (refuse) { *err = "fake: refused"; return SVO_ERR_INVALID; }
  return SVO_OK;
}
static int checked_entry(FakeCtx* ctx, bool refuse) {
  SVO_ARGS_CHECK(ctx, refuse_if(refuse, &err));
  return SVO_OK;
}

static void args_check() {
  FakeCtx ctx;
  CHECK(checked_entry(&ctx, false) == SVO_OK && ctx.err == nullptr, "an acceptance touched the context");
  CHECK(checked_entry(&ctx, true) == SVO_ERR_INVALID && ctx.err && strcmp(ctx.err, "fake: refused") == 0, "a refusal's text did not reach the context");
}

static void carve(const std::vector<size_t>& sizes, const char* where) {
  SvoParts parts;
  CHECK(parts.total() == 0, "%s: an empty layout has a size", where);
  size_t end = 0, sum = 0;
  for (size_t i = 0; i < sizes.size(); ++i) {
    const size_t before = parts.total(), at = parts.add(sizes[i]);
    CHECK(at % 256 == 0, "%s: part %zu at %zu", where, i, at);
    CHECK(at >= end, "%s: part %zu at %zu begins inside the part before it, which ends at %zu", where, i, at, end);
    CHECK(at - end < 256, "%s: part %zu at %zu leaves more than the padding behind %zu", where, i, at, end);
    if (sizes[i] == 0) CHECK(parts.total() == before, "%s: the empty part %zu took %zu bytes", where, i, parts.total() - before);
    else {
      CHECK(parts.total() >= at + sizes[i] && at + sizes[i] > at, "%s: part %zu of %zu bytes at %zu, the size is %zu", where, i, sizes[i], at, parts.total());
      end = at + sizes[i];
    }
    sum += sizes[i];
  }
  CHECK(parts.total() >= sum && parts.total() >= end, "%s: the size %zu is below the parts' sum %zu or end %zu", where, parts.total(), sum, end);
  CHECK(parts.total() - sum <= 255 * sizes.size(), "%s: the size %zu is more than the padding above the sum %zu", where, parts.total(), sum);
}

static void carver() {
  carve({}, "none");
  carve({0}, "one empty");
  carve({0, 0, 7, 0, 0}, "empties around");
  carve({1, 1, 1}, "bytes");
  carve({64, 255, 256, 257, 511, 512, 513}, "around the alignment");
  carve({48, 0, 4 * 35, 35, 0, 35}, "a 5 x 7 plan");
  const size_t big = (size_t)1 << 40;
  carve({big, big - 1, 0, big + 1, 3}, "2^40");
  static_assert(sizeof(size_t) >= 8, "the sizes are 64-bit");
  uint64_t x = 88172645463325252ull;  // xorshift: any mix of sizes
  for (int round = 0; round < 200; ++round) {
    std::vector<size_t> sizes;
    for (int i = 0; i < 12; ++i) {
      x ^= x << 13; x ^= x >> 7; x ^= x << 17;
      sizes.push_back(x % 5 == 0 ? 0 : (size_t)(x >> 8) % ((size_t)1 << (8 + 4 * (i % 9))));
    }
    carve(sizes, "random");
  }
}

int main() {
  sequence();
  args_check();
  carver();
  if (fails) { fprintf(stderr, "%d failures\n", fails); return 1; }
  printf("host call ok\n");
  return 0;
}
