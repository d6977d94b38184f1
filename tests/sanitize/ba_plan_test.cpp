// The launch planning of the device-resident window solve (stereo_vo_amd/host/ba_plan.h over csrc/lm_lds.h and csrc/lm_turns.h)
// walked on the host, under ASan + UBSan: the LDS sizes, form / k / eligibility, the compact form's waves, budget and cost, the raise
// of k with a fake occupancy and a fake ledger, and the knobs — each against a restatement written here from the rules, not by
// calling the header.
#include <limits.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>

#include "ba_plan.h"

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (++fails <= 40) { fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)

// ----------------------------------------------------------------------------- the restatements (doubles unless they say bytes)
constexpr long KIB = 1024;
static long r_even(long v) { return v + (v & 1); }
static long r_wire(int K) { const long F = K - 1; return 36 * F * (F + 1) / 2 + 33 * F + 2; }  // upper pose-pair blocks | 33 per pose | 2 scalars
static long r_ctl(int n, int K) {  // payload image | 4 vectors | term scratch | K poses twice | U staging | 8
  const long nn = std::max(n, 1);
  return (long)n * n + 3L * n + 2 + 4 * nn + nn + 14L * K + 21L * std::max(K - 1, 1) + 8;
}
static long r_tail(int n, int K) { return 3L * std::max(n, 1) + 14L * K; }
static long r_wide_area(int K) { const long E = r_wire(K); return 64 * 38 + (E <= 2048 ? r_even(E) : 0) + 2; }  // rows | partials | 4 ints
static long r_wide_union(int n, int K) { return std::max(2 * r_wide_area(K), r_ctl(n, K)); }
static long r_wide(int n, int K, int tab_words, int k) { return r_wide_union(n, K) + 2L * k * tab_words / 4 + r_tail(n, K); }
static long r_compact_area(int K) { return 64 * 38 + r_even(r_wire(K)) + 2 + 4; }
static long r_compact_union(int n, int K, int nw) { return std::max(nw * r_compact_area(K), r_ctl(n, K)); }
static long r_compact(int n, int K, int tab_words, int nw) {
  return r_compact_union(n, K, nw) + (long)nw * tab_words / 4 + 2 * r_even(r_wire(K)) + 8 + r_tail(n, K);
}
static int r_tab_words(int tab_max_words) { int w = 64; while (w < tab_max_words) w += 64; return w; }
static int r_blocks(int C, int k) { int b = 0; while (b * 2 * k < C) ++b; return b; }
static int r_cost(int grid, int per_cu, int budget_per_cu) {
  if (per_cu <= 0) return 1 << 30;
  if (per_cu >= budget_per_cu) return grid;
  int c = 0;
  while ((long)c * per_cu < (long)grid * budget_per_cu) ++c;  // ceil(grid * budget_per_cu / per_cu)
  return c;
}

static BaKnobs default_knobs() { return ba_knobs_parse([](const char*) -> const char* { return nullptr; }); }
static BaShape window(int C, int K = 5, int G = 1, int tab_max_words = 256) { return {true, C, K, 6 * (K - 1), G, 1, tab_max_words}; }

// ----------------------------------------------------------------------------- sizes
static void sizes() {
  for (int K = 1; K <= 20; ++K) {
    const int n = 6 * (K - 1);
    CHECK((long)ba_wire_elements(K) == r_wire(K), "wire elements K %d", K);
    CHECK((long)ba_lm_ctl_doubles(n, K) == r_ctl(n, K), "controller workspace K %d", K);
    CHECK((long)ba_lm_union_doubles(n, K) == r_wide_union(n, K), "wide union K %d", K);
    CHECK(ba_lm_union_doubles(n, K) == std::max((size_t)LM_CPW * (size_t)wg_lds_doubles(ba_wire_elements(K)), ba_lm_ctl_doubles(n, K)), "wide union of its parts K %d", K);
    for (int tw : {64, 256, 1024}) {
      for (int k = 1; k <= LM_MAX_WAVE_CHUNKS; ++k) {
        const size_t v = ba_lm_lds_doubles(n, K, tw, k);
        CHECK((long)v == r_wide(n, K, tw, k), "wide K %d tab %d k %d: %zu against %ld", K, tw, k, v, r_wide(n, K, tw, k));
        CHECK((long)(v - ba_lm_union_doubles(n, K) - (size_t)LM_CPW * k * tw / 4) == 3L * std::max(n, 1) + 14L * K, "wide tail K %d", K);
        if (k > 1) CHECK(v > ba_lm_lds_doubles(n, K, tw, k - 1), "wide not monotone in k: K %d tab %d k %d", K, tw, k);
      }
      for (int nw = 1; nw <= LMC_MAX_WAVES; ++nw) {
        const size_t v = ba_lmc_lds_doubles(n, K, tw, nw);
        const long Ep = r_even(r_wire(K));
        CHECK((long)v == r_compact(n, K, tw, nw), "compact K %d tab %d nw %d: %zu against %ld", K, tw, nw, v, r_compact(n, K, tw, nw));
        CHECK((long)ba_lmc_union_doubles(n, K, nw) == r_compact_union(n, K, nw), "compact union K %d nw %d", K, nw);
        CHECK(ba_lmc_union_doubles(n, K, nw) == std::max((size_t)nw * (size_t)lmc_wave_doubles(ba_wire_elements(K)), ba_lm_ctl_doubles(n, K)), "compact union of its parts K %d", K);
        CHECK((long)(v - ba_lmc_union_doubles(n, K, nw) - (size_t)nw * tw / 4) == 2 * Ep + 8 + 3L * std::max(n, 1) + 14L * K, "compact tail K %d", K);
        if (nw > 1) CHECK(v > ba_lmc_lds_doubles(n, K, tw, nw - 1), "compact not monotone in NW: K %d tab %d nw %d", K, tw, nw);
      }
    }
  }
  // n = 36, K = 7 by hand: F = 6, E = 18 * 6 * 7 + 33 * 6 + 2 = 956; a wavefront's area 64 * 38 + 956 + 2 = 3,390, two of them 6,780; the
  // controller 1,296 + 108 + 2 + 144 + 36 + 98 + 126 + 8 = 1,818: the union is 6,780.  Tables of 256 words: 2 k * 64 doubles.  Tail
  // 3 * 36 + 14 * 7 = 206.  k = 1: 6,780 + 128 + 206 = 7,114 (the allocation that was once 36 short said 7,078); k = 3: 7,370.
  CHECK(ba_lm_lds_doubles(36, 7, 256, 1) == 7114, "n = 36, K = 7, k = 1: %zu", ba_lm_lds_doubles(36, 7, 256, 1));
  CHECK(ba_lm_lds_doubles(36, 7, 256, 3) == 7370, "n = 36, K = 7, k = 3: %zu", ba_lm_lds_doubles(36, 7, 256, 3));
  for (int w : {0, 1, 63, 64, 65, 128, 129, 1000, 1024, 1025, 4096}) CHECK(ba_plan_tab_words(w) == r_tab_words(w), "tab words of %d", w);
}

// ----------------------------------------------------------------------------- form, k, eligibility of the wide form
static void wide_form() {
  BaKnobs kn = default_knobs();
  for (int C = 1; C <= 300; ++C)
    for (int G = 1; G <= 2; ++G)
      for (int own = 0; own <= 8; ++own)
        for (int knob = 1; knob <= 8; ++knob)
          for (int request = 0; request <= 1; ++request) {
            kn.wave_chunks = knob;
            BaOverrides ov;
            ov.lm_wave_chunks = own;
            ov.device_lm = request ? 1 : -1;
            const BaShape s = window(C, 5, G);
            const int k = (G > 1 || C <= 2) ? 1 : (own > 0 ? own : knob);
            const int form = G > 1 ? BA_FORM_GROUPED : (k > 1 ? BA_FORM_MULTI : BA_FORM_PLAIN);
            const bool ok = C <= 288 && (G == 1 || request);  // (K = 5, tables of 256 words: 30 KiB at k = 8)
            BaWidePlan p;
            const bool got = ba_plan_wide(s, ov, kn, &p);
            CHECK(ba_plan_k(s, ov, kn) == k && p.k == k && p.form == form && ba_plan_wide_form(s, k) == form, "C %d G %d own %d knob %d: k %d form %d", C, G, own, knob, p.k, p.form);
            CHECK(got == ok, "C %d G %d own %d knob %d request %d: eligible %d", C, G, own, knob, request, (int)got);
            if (got) CHECK((long)p.lds == 8 * r_wide(24, 5, 256, k) && p.blocks == r_blocks(C, k) && p.yield_after == 0, "C %d k %d: lds %zu blocks %d", C, k, p.lds, p.blocks);
          }
  // each boundary at its limit and one beyond
  kn = default_knobs();
  BaOverrides ov, req;
  req.device_lm = 1;
  BaWidePlan p;
  auto eligible = [&](BaShape s, const BaOverrides& o) { return ba_plan_wide(s, o, kn, &p); };
  CHECK(eligible(window(288, 5, 2), req) && !eligible(window(289, 5, 2), req), "C 288 / 289");
  BaShape s = window(100);
  CHECK(eligible(s, ov), "a window");
  s.det = false; CHECK(!eligible(s, ov), "not deterministic"); s.det = true;
  s.C = 0; CHECK(!eligible(s, ov), "no chunks"); s.C = 100;
  s.CPW = 2; CHECK(!eligible(s, ov), "CPW 2"); s.CPW = 1;
  s.tab_max_words = 1024; CHECK(eligible(s, ov) && (long)p.lds == 8 * r_wide(24, 5, 1024, 3), "table words 1024");
  s.tab_max_words = 1025; CHECK(!eligible(s, ov), "table words 1025");
  CHECK(!eligible(window(200, 5, 2), ov) && eligible(window(200, 5, 2), req), "grouped without and with request");
  ov.device_lm = 0; CHECK(!eligible(window(200, 5, 2), ov), "grouped, device solve off"); ov.device_lm = -1;
  // the first (n, k) at which the LDS passes 120 KiB: for every k the largest K that fits, and K + 1 refused
  int n_fit = 0, n_refused = 0;
  for (int k = 1; k <= LM_MAX_WAVE_CHUNKS; ++k) {
    BaOverrides o;
    o.lm_wave_chunks = k;
    int last_fit = 0;
    for (int K = 2; K <= 24; ++K) {
      const bool fits = 8 * r_wide(6 * (K - 1), K, 1024, k) <= 120 * KIB;
      const bool got = eligible(window(100, K, 1, 1024), o);
      CHECK(got == fits, "K %d k %d: %ld bytes, eligible %d", K, k, 8 * r_wide(6 * (K - 1), K, 1024, k), (int)got);
      if (fits) { CHECK(last_fit == K - 1 || last_fit == 0, "K %d k %d fits behind one that does not", K, k); last_fit = K; ++n_fit; } else ++n_refused;
    }
    CHECK(last_fit >= 2 && last_fit < 24, "k %d: the 120 KiB boundary lies outside K 2..24", k);
  }
  CHECK(n_fit > 0 && n_refused > 0, "120 KiB boundary not reached");
  // yield iterations: the adjuster's, else the knob, only beyond k = 1
  kn.yield_iters = 4;
  CHECK(eligible(window(100), ov) && p.yield_after == 4, "yield from the knob");
  ov.yield_iters = 0; CHECK(eligible(window(100), ov) && p.yield_after == 0, "yield 0 of the adjuster");
  ov.yield_iters = 2; CHECK(eligible(window(100), ov) && p.yield_after == 2, "yield of the adjuster");
  CHECK(eligible(window(2), ov) && p.k == 1 && p.yield_after == 0, "k = 1 never yields");
  // the device solve: the adjuster's switch, else the knob, else the throughput mode
  BaOverrides d;
  CHECK(ba_plan_device_lm(d, kn) == -1, "device solve unset");
  kn.device_lm = 0; CHECK(ba_plan_device_lm(d, kn) == 0, "device solve off by the knob");
  d.device_lm = 1; CHECK(ba_plan_device_lm(d, kn) == 1, "device solve on by the adjuster");
  d.device_lm = 0; kn.device_lm = 1; CHECK(ba_plan_device_lm(d, kn) == 0, "device solve off by the adjuster");
}

// ----------------------------------------------------------------------------- the compact form
static void compact_form() {
  BaKnobs kn = default_knobs();
  auto waves = [&](const BaShape& s) { return ba_plan_compact_waves(s, kn.compact_waves); };  // 0: not eligible
  CHECK(waves(window(256)) == 6 && waves(window(257)) == 0, "compact C 256 / 257");
  const int w4096 = waves(window(50, 5, 1, 4096));  // (tables of 1,024 doubles per wave: fewer than six fit)
  CHECK(w4096 >= 1 && w4096 < 6 && 8 * r_compact(24, 5, 4096, w4096) <= 156 * KIB && 8 * r_compact(24, 5, 4096, w4096 + 1) > 156 * KIB, "compact table words 4096: %d waves", w4096);
  CHECK((long)ba_plan_compact_lds(window(50, 5, 1, 4096), w4096) == 8 * r_compact(24, 5, 4096, w4096), "compact table words 4096: lds");
  CHECK(waves(window(50, 5, 1, 4097)) == 0, "compact table words 4097");
  BaShape s = window(50);
  s.det = false; CHECK(waves(s) == 0, "compact, not deterministic"); s.det = true;
  s.C = 0; CHECK(waves(s) == 0, "compact, no chunks");
  int k_one = 0;  // the largest K at which one wave still fits
  for (int K = 2; K <= 40; ++K) if (8 * r_compact(6 * (K - 1), K, 256, 1) <= 156 * KIB) k_one = K;
  CHECK(k_one >= 10 && k_one < 39, "the 156 KiB boundary of one wave lies at K %d", k_one);
  int n_less = 0;
  for (int cap = 1; cap <= 6; ++cap)
    for (int C = 1; C <= 10; ++C)
      for (int K = 2; K <= k_one + 1; ++K) {
        int want = 0;
        for (int nw = 1; nw <= std::min(cap, std::max(1, C)); ++nw) if (8 * r_compact(6 * (K - 1), K, 256, nw) <= 156 * KIB) want = nw;
        const int got = ba_plan_compact_waves(window(C, K), cap);
        CHECK(got == want, "cap %d C %d K %d: waves %d, wanted %d", cap, C, K, got, want);
        if (got) CHECK((long)ba_plan_compact_lds(window(C, K), got) == 8 * r_compact(6 * (K - 1), K, 256, want), "cap %d C %d K %d: lds", cap, C, K);
        if (want >= 1 && want < std::min(cap, C)) ++n_less;
        if (K == k_one + 1) CHECK(got == 0, "K %d fits no wave", K);
      }
  CHECK(n_less > 0, "no case where the LDS budget decides the waves");
  // a launch of several: the smallest wave count of its solves, the largest LDS at that count
  const BaShape mixed[4] = {window(40, 5), window(3, 4), window(60, 11, 1, 1000), window(9, 7)};
  int plans[4];
  for (int count = 1; count <= 4; ++count) {
    int nw = 6;
    long lds = 0;
    for (int i = 0; i < count; ++i) { plans[i] = waves(mixed[i]); CHECK(plans[i] >= 1, "mixed solve %d", i); nw = std::min(nw, plans[i]); }
    for (int i = 0; i < count; ++i) lds = std::max(lds, 8 * r_compact(mixed[i].n, mixed[i].K, r_tab_words(mixed[i].tab_max_words), nw));
    const BaCompactLaunch l = ba_plan_compact_launch(mixed, plans, count);
    CHECK(l.waves == nw && (long)l.lds == lds && l.lds <= LMC_LDS_BUDGET, "launch of %d: waves %d lds %zu, wanted %d %ld", count, l.waves, l.lds, nw, lds);
  }
  CHECK(plans[0] == 6 && plans[1] == 3 && plans[2] < 6, "the mixed set does not mix: %d %d %d", plans[0], plans[1], plans[2]);
  // which form a solve asks for: the penalty, then the adjuster's form, then the knob; a solve that yielded stays wide
  kn = default_knobs();
  for (int penalty : {0, 3})
    for (int form : {-1, 0, 1})
      for (int knob : {-1, 0, 1})
        for (int yielded = 0; yielded <= 1; ++yielded) {
          BaOverrides ov;
          ov.lm_penalty = penalty; ov.lm_form = form;
          kn.form = knob;
          const bool want = !yielded && (penalty > 0 || (form >= 0 ? form == 1 : knob == 1));
          CHECK(ba_plan_wants_compact(ov, kn, yielded != 0) == want, "penalty %d form %d knob %d yielded %d", penalty, form, knob, yielded);
        }
}

// ----------------------------------------------------------------------------- budget and cost
static int r_budget(int per_cu, int cus, int share, int percent) {
  const int usable = per_cu >= 3 ? per_cu - 1 : (per_cu >= 1 ? 1 : 0);
  int b = usable * cus;
  b /= 8; b *= 7; b *= share; b /= 32;
  if (percent >= 10 && percent <= 400) b = (int)((long long)b * percent / 100);
  return b;
}
static void budget_and_cost() {
  for (int per_cu = 0; per_cu <= 6; ++per_cu) {
    for (int bpc = 1; bpc <= 6; ++bpc)
      for (int grid = 1; grid <= 150; ++grid) {
        const int c = ba_plan_cost(grid, per_cu, bpc);
        CHECK(c == r_cost(grid, per_cu, bpc), "cost grid %d per_cu %d budget_per_cu %d: %d", grid, per_cu, bpc, c);
        CHECK(c >= grid, "a workgroup never costs less than one");
      }
    for (int cus : {1, 8, 104, 256})
      for (int share : {32, 16})
        for (int percent : {0, 9, 10, 50, 100, 150, 400, 401})
          CHECK(ba_plan_budget(per_cu, cus, share, percent) == r_budget(per_cu, cus, share, percent), "budget per_cu %d cus %d share %d percent %d", per_cu, cus, share, percent);
  }
  // 256 CUs at 4 per CU: 3 usable, 768 / 8 * 7 = 672
  CHECK(ba_plan_budget(4, 256, 32, 0) == 672 && ba_plan_budget(4, 256, 16, 0) == 336, "share 32 / 16");
  CHECK(ba_plan_budget(4, 256, 32, 9) == 672 && ba_plan_budget(4, 256, 32, 10) == 67 && ba_plan_budget(4, 256, 32, 400) == 2688 && ba_plan_budget(4, 256, 32, 401) == 672, "percent 9 / 10 / 400 / 401");
  CHECK(ba_plan_budget(2, 256, 32, 0) == 224 && ba_plan_budget(1, 256, 32, 0) == 224 && ba_plan_budget(0, 256, 32, 0) == 0, "usable workgroups per CU");
}

// ----------------------------------------------------------------------------- raising k
static void raise_k() {
  const BaKnobs kn = default_knobs();
  const int K = 5, n = 24, tab = 256;
  long n_raised = 0, n_dropped = 0, n_unsaved = 0;
  for (int k0 : {2, 3})
    for (int bpc : {2, 3})
      for (int drop_k = k0; drop_k <= LM_MAX_WAVE_CHUNKS + 1; ++drop_k)  // the occupancy is 2 up to the LDS of drop_k, 1 beyond (9: never drops)
        for (int allow_k : {LM_MAX_WAVE_CHUNKS, 5})                       // the dynamic-LDS limit cannot be raised beyond the LDS of allow_k
         for (int recovers = 0; recovers <= 1; ++recovers)                // ... 1: both only up to the LDS of the next k (a stop is a stop, not a skip)
          for (int C = 3; C <= 256; ++C) {
            const long drop_lds = 8 * r_wide(n, K, tab, std::min(drop_k, LM_MAX_WAVE_CHUNKS)) + (drop_k > LM_MAX_WAVE_CHUNKS ? 8 : 0);
            const long allow_lds = 8 * r_wide(n, K, tab, allow_k);
            const long step = 8 * (r_wide(n, K, tab, 2) - r_wide(n, K, tab, 1));  // bytes of LDS from one k to the next
            auto occupancy = [&](long lds) { return lds > drop_lds && !(recovers && lds > drop_lds + step) ? 1 : 2; };
            auto allowed = [&](long lds) { return lds <= allow_lds || (recovers && lds > allow_lds + step); };
            const int top = r_cost(r_blocks(C, k0), 2, bpc);
            for (int B = 0; B <= top; ++B) {  // (B = top admits at k0: the caller would not raise; as a remaining budget it is as good as any)
              // restated: the smallest k beyond k0 that saves a workgroup against k - 1 and whose cost fits B, provided that every k that
              // saves a workgroup up to it keeps the occupancy and may be launched
              int want = 0, want_offers = 0;
              for (int k = k0 + 1; k <= LM_MAX_WAVE_CHUNKS && !want; ++k) {
                if (r_blocks(C, k) == r_blocks(C, k - 1)) { ++n_unsaved; continue; }
                const long lds = 8 * r_wide(n, K, tab, k);
                if (lds > 120 * KIB || occupancy(lds) < 2 || !allowed(lds)) { ++n_dropped; break; }
                ++want_offers;
                if (r_cost(r_blocks(C, k), 2, bpc) <= B) want = k;
              }
              BaOverrides ov;
              BaKnobs knobs = kn;
              knobs.wave_chunks = k0;
              const BaShape s = window(C, K, 1, tab);
              BaWidePlan p;
              if (!ba_plan_wide(s, ov, knobs, &p)) { CHECK(false, "C %d not eligible", C); continue; }
              if (p.form != BA_FORM_MULTI) { CHECK(C <= 2, "C %d at k %d is not the multi form", C, k0); continue; }
              int offers = 0, last_cost = INT_MAX;
              bool offered_past_drop = false, saw_stop = false;  // (a stop: an occupancy below the first one, or an LDS that is not allowed)
              size_t seen_lds = 0;
              const BaWidePlan before = p;
              const bool got = ba_plan_raise_k(
                  s, ov, bpc, &p, [&](size_t lds) { seen_lds = lds; saw_stop |= occupancy((long)lds) < 2; return occupancy((long)lds); },
                  [&](size_t lds) { saw_stop |= !allowed((long)lds); return allowed((long)lds); },
                  [&](int cost) {
                    ++offers;
                    if (saw_stop || (!recovers && (long)seen_lds > drop_lds)) offered_past_drop = true;
                    CHECK(cost < last_cost, "C %d k0 %d: an offer of %d behind one of %d saves nothing", C, k0, cost, last_cost);
                    last_cost = cost;
                    return cost <= B;
                  });
              CHECK(got == (want != 0) && (got ? p.k == want : p.k == before.k), "C %d k0 %d budget_per_cu %d drop %d allow %d B %d: k %d, wanted %d", C, k0, bpc, drop_k, allow_k, B, got ? p.k : 0, want);
              CHECK(offers == want_offers, "C %d k0 %d drop %d B %d: %d offers, wanted %d", C, k0, drop_k, B, offers, want_offers);
              CHECK(!offered_past_drop, "C %d k0 %d drop %d: offered behind the occupancy drop", C, k0, drop_k);
              if (got) {
                ++n_raised;
                CHECK((long)p.lds == 8 * r_wide(n, K, tab, want) && p.blocks == r_blocks(C, want) && p.form == BA_FORM_MULTI, "C %d: the raised plan", C);
                // no admissible smaller k was skipped
                for (int k = k0 + 1; k < want; ++k)
                  CHECK(r_blocks(C, k) == r_blocks(C, k - 1) || r_cost(r_blocks(C, k), 2, bpc) > B, "C %d B %d: k %d was admissible, %d taken", C, B, k, want);
              } else {
                CHECK(p.lds == before.lds && p.blocks == before.blocks, "C %d: a refused plan changed", C);
              }
              // an adjuster with its own k is never raised, nor is anything offered for it
              BaOverrides own;
              own.lm_wave_chunks = k0;
              BaWidePlan q;
              int own_offers = 0;
              CHECK(ba_plan_wide(s, own, knobs, &q) && q.k == k0, "C %d: own k", C);
              CHECK(!ba_plan_raise_k(s, own, bpc, &q, [&](size_t) { return 2; }, [&](size_t) { return true; }, [&](int) { ++own_offers; return true; }) && own_offers == 0 && q.k == k0,
                    "C %d: an adjuster with its own k was raised", C);
            }
          }
  CHECK(n_raised > 1000 && n_dropped > 1000 && n_unsaved > 1000, "raise k: %ld raised, %ld stopped, %ld skipped: a branch is hardly reached", n_raised, n_dropped, n_unsaved);
  // an unknown occupancy at the offered k, the plain and the grouped form: nothing is offered
  int offers = 0;
  auto count = [&](int) { ++offers; return true; };
  BaOverrides ov;
  BaWidePlan p;
  CHECK(ba_plan_wide(window(100), ov, kn, &p) && !ba_plan_raise_k(window(100), ov, 2, &p, [](size_t) { return 0; }, [](size_t) { return true; }, count) && offers == 0, "unknown occupancy");
  CHECK(ba_plan_wide(window(2), ov, kn, &p) && p.form == BA_FORM_PLAIN && !ba_plan_raise_k(window(2), ov, 2, &p, [](size_t) { return 2; }, [](size_t) { return true; }, count) && offers == 0, "plain form");
  ov.device_lm = 1;
  CHECK(ba_plan_wide(window(200, 5, 2), ov, kn, &p) && p.form == BA_FORM_GROUPED && !ba_plan_raise_k(window(200, 5, 2), ov, 2, &p, [](size_t) { return 2; }, [](size_t) { return true; }, count) && offers == 0, "grouped form");
}

// ----------------------------------------------------------------------------- knobs
static BaKnobs parse(const char* name, const char* value) {
  return ba_knobs_parse([&](const char* q) -> const char* { return value && strcmp(q, name) == 0 ? value : nullptr; });
}
static void knobs() {
  const BaKnobs d = default_knobs();
  CHECK(d.wave_chunks == 3 && !d.wave_contig && d.compact_waves == 6 && d.form == -1 && d.yield_iters == 0 && !d.overflow && d.device_lm == -1 && d.budget_percent == 0, "defaults");
  // the one parser: unset, empty, in range, below, above, non-numeric
  CHECK(ba_env_int(nullptr, 3, 1, 8) == 3 && ba_env_int("", 3, 1, 8) == 3 && ba_env_int("5", 3, 1, 8) == 5 && ba_env_int("0", 3, 1, 8) == 1 && ba_env_int("-4", 3, 1, 8) == 1 &&
            ba_env_int("9", 3, 1, 8) == 8 && ba_env_int("many", 3, 1, 8) == 1 && ba_env_int("1", 3, 1, 8) == 1 && ba_env_int("8", 3, 1, 8) == 8,
        "integer with default and clamp");
  struct Case { const char* value; int want; };
  const char* name = "SVO_BA_WAVE_CHUNKS";
  for (Case c : {Case{nullptr, 3}, {"", 3}, {"1", 1}, {"4", 4}, {"8", 8}, {"0", 1}, {"-2", 1}, {"9", 8}, {"100", 8}, {"k", 1}}) CHECK(parse(name, c.value).wave_chunks == c.want, "%s=%s", name, c.value ? c.value : "(unset)");
  name = "SVO_BA_COMPACT_WAVES";
  for (Case c : {Case{nullptr, 6}, {"", 6}, {"1", 1}, {"3", 3}, {"6", 6}, {"0", 1}, {"-2", 1}, {"7", 6}, {"k", 1}}) CHECK(parse(name, c.value).compact_waves == c.want, "%s=%s", name, c.value ? c.value : "(unset)");
  name = "SVO_BA_YIELD_ITERS";
  for (Case c : {Case{nullptr, 0}, {"", 0}, {"0", 0}, {"2", 2}, {"1000", 1000}, {"-1", 0}, {"k", 0}}) CHECK(parse(name, c.value).yield_iters == c.want, "%s=%s", name, c.value ? c.value : "(unset)");
  name = "SVO_BA_OVERFLOW";
  for (Case c : {Case{nullptr, 0}, {"", 0}, {"0", 0}, {"1", 1}, {"2", 1}, {"-1", 1}, {"k", 0}}) CHECK((int)parse(name, c.value).overflow == c.want, "%s=%s", name, c.value ? c.value : "(unset)");
  name = "SVO_BA_DEVICE_LM";
  for (Case c : {Case{nullptr, -1}, {"", -1}, {"0", 0}, {"1", 1}, {"2", 1}, {"-1", 1}, {"k", 0}}) CHECK(parse(name, c.value).device_lm == c.want, "%s=%s", name, c.value ? c.value : "(unset)");
  name = "SVO_BA_BUDGET_PERCENT";
  for (Case c : {Case{nullptr, 0}, {"", 0}, {"9", 9}, {"10", 10}, {"400", 400}, {"401", 401}, {"k", 0}}) {
    const int pct = parse(name, c.value).budget_percent;
    CHECK(pct == c.want && ba_plan_budget(4, 256, 32, pct) == (pct >= 10 && pct <= 400 ? 672 * pct / 100 : 672), "%s=%s", name, c.value ? c.value : "(unset)");
  }
  name = "SVO_BA_FORM";
  for (Case c : {Case{nullptr, -1}, {"", -1}, {"compact", 1}, {"c", 1}, {"wide", 0}, {"w", 0}, {"1", -1}, {"Compact", -1}}) CHECK(parse(name, c.value).form == c.want, "%s=%s", name, c.value ? c.value : "(unset)");
  name = "SVO_BA_WAVE_ORDER";
  for (Case c : {Case{nullptr, 0}, {"", 0}, {"contiguous", 1}, {"c", 1}, {"strided", 0}, {"1", 0}}) CHECK((int)parse(name, c.value).wave_contig == c.want, "%s=%s", name, c.value ? c.value : "(unset)");
  // one variable moves one field
  const BaKnobs o = parse("SVO_BA_OVERFLOW", "1");
  CHECK(o.wave_chunks == 3 && o.compact_waves == 6 && o.form == -1 && o.yield_iters == 0 && o.device_lm == -1 && o.budget_percent == 0 && !o.wave_contig, "one variable, one field");
}

int main() {
  sizes();
  wide_form();
  compact_form();
  budget_and_cost();
  raise_k();
  knobs();
  if (fails) { fprintf(stderr, "%d checks failed\n", fails); return 1; }
  printf("ba plan ok\n");
  return 0;
}
