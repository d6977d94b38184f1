// How a device-resident window solve is planned before it is launched (csrc/ba.hip, ba_device_lm_launch), free of the
// GPU: the process knobs, whether a loaded problem is eligible, which form it takes (ba_lm_kernel, ba_lm_grouped_kernel,
// ba_lm_multi_kernel, ba_lm_compact_kernel), chunks per wavefront k, dynamic LDS and workgroups, what the launch costs in the
// admission budget, to which larger k a refused solve is raised, and the wavefronts of a compact solve.  Functions of plain values;
// ba.hip keeps the occupancy queries, hipFuncSetAttribute, the ledger and the launches, and has no second copy of anything here.
// tests/sanitize/ba_plan_test.cpp walks every rule against a brute-force restatement on a CPU.
#ifndef SVO_BA_PLAN_H_
#define SVO_BA_PLAN_H_
#include <limits.h>
#include <stddef.h>
#include <stdlib.h>

#include "lm_lds.h"
#include "lm_turns.h"

// ----------------------------------------------------------------------------- knobs: the process's, one adjuster's
// The one parser of "integer from the environment": unset or empty gives the default, anything else atoi's value, clamped to lo..hi.
inline int ba_env_int(const char* s, int dflt, int lo, int hi) { const int v = s && *s ? atoi(s) : dflt; return v < lo ? lo : (v > hi ? hi : v); }

constexpr int LM_WAVE_CHUNKS_DEFAULT = 3;
struct BaKnobs {
  int wave_chunks;     // SVO_BA_WAVE_CHUNKS=1..LM_MAX_WAVE_CHUNKS (developer knob): the k a wide solve is offered to the admission with
  bool wave_contig;    // SVO_BA_WAVE_ORDER=contiguous gives a wavefront neighbouring chunks instead of one per stride (see lm_turns.h)
  int compact_waves;   // SVO_BA_COMPACT_WAVES=1..LMC_MAX_WAVES: the most wavefronts a compact solve gets
  int form;            // SVO_BA_FORM=compact: 1, wide: 0, else -1
  int yield_iters;     // SVO_BA_YIELD_ITERS: LM iterations a wide solve runs per launch before it steps aside (0: never)
  // SVO_BA_OVERFLOW=1: a solve the admission budget refuses takes the compact form at once instead of waiting for the budget.  Off by
  // default: measured in round 5 (profiles/r05_exp_lanes_groups.txt) it helps only while streams share hardware queues (7 lines per group
  // on 16 queues: 30 k against 25 k frames/s at 128 lanes); with one hardware queue per stream the wide form alone is faster (37-51 k
  // against 27-36 k) — a 3 ms compact solve holds its line for 3 ms.
  bool overflow;
  int device_lm;       // SVO_BA_DEVICE_LM=0 / 1 forces; -1 (unset): follow svo_throughput_mode()
  int budget_percent;  // SVO_BA_BUDGET_PERCENT, developer experiments (profiles/r04_exp_admission_budget.txt): honoured in 10..400 only
};
template <class Env>  // const char* env(const char* name): getenv, or a test's table
BaKnobs ba_knobs_parse(Env env) {
  BaKnobs k;
  const char *order = env("SVO_BA_WAVE_ORDER"), *form = env("SVO_BA_FORM"), *dlm = env("SVO_BA_DEVICE_LM");
  k.wave_chunks = ba_env_int(env("SVO_BA_WAVE_CHUNKS"), LM_WAVE_CHUNKS_DEFAULT, 1, LM_MAX_WAVE_CHUNKS);
  k.wave_contig = order && order[0] == 'c';
  k.compact_waves = ba_env_int(env("SVO_BA_COMPACT_WAVES"), LMC_MAX_WAVES, 1, LMC_MAX_WAVES);
  k.form = !form ? -1 : (form[0] == 'c' ? 1 : (form[0] == 'w' ? 0 : -1));
  k.yield_iters = ba_env_int(env("SVO_BA_YIELD_ITERS"), 0, 0, INT_MAX);
  k.overflow = ba_env_int(env("SVO_BA_OVERFLOW"), 0, INT_MIN, INT_MAX) != 0;
  k.device_lm = dlm && *dlm ? (ba_env_int(dlm, 0, INT_MIN, INT_MAX) != 0 ? 1 : 0) : -1;
  k.budget_percent = ba_env_int(env("SVO_BA_BUDGET_PERCENT"), 0, INT_MIN, INT_MAX);
  return k;
}
inline const BaKnobs& ba_knobs() { static const BaKnobs k = ba_knobs_parse(getenv); return k; }  // read once per process

// What one adjuster sets for its own solves, over the process's knobs.
struct BaOverrides {
  int lm_wave_chunks = 0;  // svo_ba_set_wave_chunks: chunks per wavefront of this adjuster's wide solves (0: the process default, raised where the admission budget asks for it)
  int lm_form = -1;        // svo_ba_set_solve_form: which device-resident form — 0 wide (ba_lm_kernel: many workgroups, lowest latency), 1 compact (ba_lm_compact_kernel: one workgroup, smallest footprint), -1 automatic (SVO_BA_FORM, else wide)
  int lm_penalty = 0;      // solves left that avoid the wide form after one of its launches gave up
  int yield_iters = -1;    // svo_ba_set_yield_iterations: LM iterations per launch (0: never yields, -1: SVO_BA_YIELD_ITERS, else 0)
  int device_lm = -1;      // svo_ba_set_device_lm: -1 automatic, 0 never, 1 whenever eligible
};

// 1: the device-resident solve is on for this adjuster, 0: off, -1: it follows svo_throughput_mode()
inline int ba_plan_device_lm(const BaOverrides& ov, const BaKnobs& kn) { return ov.device_lm >= 0 ? ov.device_lm : kn.device_lm; }

// ----------------------------------------------------------------------------- the loaded problem
// det: deterministic mode; C chunks, K keyframes, n = 6 (K - 1) the reduced camera system's dimension, G chunks per declared group (> 1:
// more than 128 chunks), CPW chunks per stored partial, tab_max_words the largest chunk table (u16 words)
struct BaShape { bool det; int C, K, n, G, CPW, tab_max_words; };
// u16 words per chunk table in LDS, either form
inline int ba_plan_tab_words(int tab_max_words) { const int w = (tab_max_words + 63) & ~63; return w < 64 ? 64 : w; }

// ----------------------------------------------------------------------------- the wide form
// Chunks per wavefront a wide solve is offered to the admission with (ba_lm_multi_kernel for more than one; a solve the budget
// refuses at this k is offered again at larger ones, see ba_plan_raise_k).  Windows of more than 128 chunks (ba_lm_grouped_kernel)
// keep one chunk per wavefront; so do solves of no more than two chunks (one workgroup either way).
inline int ba_plan_k(const BaShape& s, const BaOverrides& ov, const BaKnobs& kn) { return s.G > 1 || s.C <= LM_CPW ? 1 : (ov.lm_wave_chunks > 0 ? ov.lm_wave_chunks : kn.wave_chunks); }
// windows of up to 128 chunks: ba_lm_kernel, or ba_lm_multi_kernel (several chunks per wavefront); beyond: ba_lm_grouped_kernel
enum { BA_FORM_PLAIN = 0, BA_FORM_GROUPED = 1, BA_FORM_MULTI = 2, BA_WIDE_FORMS = 3 };
inline int ba_plan_wide_form(const BaShape& s, int k) { return s.G > 1 ? BA_FORM_GROUPED : (k > 1 ? BA_FORM_MULTI : BA_FORM_PLAIN); }

constexpr size_t LM_LDS_LIMIT = 120 * 1024;  // dynamic LDS of a wide solve: n <= 100 or so; window problems are n <= 60
constexpr int LM_MAX_CHUNKS_GROUPED = 288;   // wide form: 129..288 chunks go to ba_lm_grouped_kernel (144 workgroups at one per CU fit the admission budget)
inline size_t ba_plan_wide_lds(const BaShape& s, int k) { return sizeof(double) * ba_lm_lds_doubles(s.n, s.K, ba_plan_tab_words(s.tab_max_words), k); }

// form: BA_FORM_*, k: chunks per wavefront, lds: bytes of dynamic LDS, blocks: workgroups, yield_after: LM iterations per launch
// (ba_lm_multi_kernel only; 0: never) — the adjuster's, else SVO_BA_YIELD_ITERS, else never
struct BaWidePlan { int form, k; size_t lds; int blocks, yield_after; };
// Always fills form and k (which launch the solve belongs to); false: not eligible (the host-driven path takes it).
inline bool ba_plan_wide(const BaShape& s, const BaOverrides& ov, const BaKnobs& kn, BaWidePlan* p) {
  const int k = ba_plan_k(s, ov, kn);
  *p = {ba_plan_wide_form(s, k), k, 0, 0, 0};
  // every chunk table in LDS, every chunk its own partial (beyond 128 chunks the grouped kernel sums groups of G chunks first), and
  // the launch must fit the admission budget at all (workgroups that wait for each other): window-sized problems
  if (!s.det || s.C <= 0 || s.C > LM_MAX_CHUNKS_GROUPED || s.CPW != 1 || s.tab_max_words > TAB_LDS_WORDS) return false;
  // beyond 128 chunks (ba_lm_grouped_kernel) only on request: measured on configs[2]'s 10-keyframe windows (~210 chunks, E = 2,312 wire
  // elements) the host-driven loop is faster — 780 against 590 frames/s (profiles/r05_exp_single_stream_paths.txt)
  if (s.G > 1 && ov.device_lm != 1) return false;
  p->lds = ba_plan_wide_lds(s, k);
  if (p->lds > LM_LDS_LIMIT) return false;
  p->blocks = ba_lm_blocks(s.C, k);
  p->yield_after = k > 1 ? (ov.yield_iters >= 0 ? ov.yield_iters : kn.yield_iters) : 0;
  return true;
}

// ----------------------------------------------------------------------------- the compact form
// the waves per workgroup that fit 156 KB of dynamic LDS (the kernel keeps ~1.5 KB of static LDS), at most SVO_BA_COMPACT_WAVES
// (default 6) and not more than the problem has chunks; 0: not eligible
constexpr size_t LMC_LDS_BUDGET = 156 * 1024;
constexpr int LMC_MAX_CHUNKS = 256;   // beyond, a single workgroup's rounds take longer than the host-driven loop's launches
constexpr int LMC_MAX_TAB_WORDS = 4096;
inline size_t ba_plan_compact_lds(const BaShape& s, int nw) { return sizeof(double) * ba_lmc_lds_doubles(s.n, s.K, ba_plan_tab_words(s.tab_max_words), nw); }
inline int ba_plan_compact_waves(const BaShape& s, int cap) {
  if (!s.det || s.C <= 0 || s.C > LMC_MAX_CHUNKS || s.tab_max_words > LMC_MAX_TAB_WORDS) return 0;
  int nw = cap < s.C ? cap : s.C;
  while (nw >= 1 && ba_plan_compact_lds(s, nw) > LMC_LDS_BUDGET) --nw;
  return nw;
}
// one launch = one workgroup shape: the smallest wave count of its solves (fewer waves need less LDS), LDS of the largest
struct BaCompactLaunch { int waves; size_t lds; };
inline BaCompactLaunch ba_plan_compact_launch(const BaShape* s, const int* waves, int count) {
  BaCompactLaunch l = {LMC_MAX_WAVES, 0};
  for (int i = 0; i < count; ++i) if (waves[i] < l.waves) l.waves = waves[i];
  for (int i = 0; i < count; ++i) { const size_t lds = ba_plan_compact_lds(s[i], l.waves); if (lds > l.lds) l.lds = lds; }
  return l;
}

// which device-resident form a solve takes (see svo_ba_set_solve_form); a solve that stepped aside (yielded) goes on in the wide form
inline bool ba_plan_wants_compact(const BaOverrides& ov, const BaKnobs& kn, bool yielded) {
  if (yielded) return false;
  if (ov.lm_penalty > 0) return true;
  if (ov.lm_form >= 0) return ov.lm_form == 1;
  return kn.form == 1;
}

// ----------------------------------------------------------------------------- the admission budget and what a launch costs in it
// Workgroups of waiting kernels the process admits at once: 7/8 of what the device holds of ba_lm_kernel at the window-5 problem's
// LDS (per_cu workgroups on each of cus CUs), scaled by the CUs of every 32 the adjusters' streams may use and by `percent`.
inline int ba_plan_budget(int per_cu, int cus, int cu_share, int percent) {
  // LDS is handed out in contiguous pieces: between the tracker's small workgroups a CU may not have room for the last
  // workgroup the occupancy query promises, so one per CU is left out of the count
  const int usable = per_cu >= 3 ? per_cu - 1 : (per_cu >= 1 ? 1 : 0);
  int budget = usable * cus / 8 * 7 * cu_share / 32;  // a CU-masked stream holds proportionally fewer workgroups
  if (percent >= 10 && percent <= 400) budget = (int)((long long)budget * percent / 100);
  return budget;
}
// What `grid` workgroups of a kernel that fits per_cu of them on a CU cost in the units of that budget (budget_per_cu on a CU): a
// larger reduced camera system (10-keyframe windows) lowers the kernel's occupancy, its workgroups then count for more.
inline int ba_plan_cost(int grid, int per_cu, int budget_per_cu) {
  if (per_cu <= 0) return 1 << 30;
  if (per_cu >= budget_per_cu) return grid;
  return (grid * budget_per_cu + per_cu - 1) / per_cu;
}

// The budget refuses the solve at the k it was offered with: it rides this launch on fewer workgroups — the first larger k that fits, as
// long as the kernel's workgroups per CU at that k's LDS (k chunk tables per wavefront) stay what they are at the offered k, so
// that the launch's dynamic LDS (the maximum over its solves) takes no residency from the solves beside it.  Same kernel, same
// hand-overs, every chunk posts its own partials: the same bits.  What is charged is the cost at the k and the LDS it runs with.
// Only ba_lm_multi_kernel's solves, and only where the adjuster has no k of its own.  per_cu(lds): workgroups per CU at lds bytes (0:
// unknown); allow(lds): the kernel may be launched with that much; admit(cost): the ledger takes it.  true: *p is the admitted plan.
template <class PerCu, class Allow, class Admit>
bool ba_plan_raise_k(const BaShape& s, const BaOverrides& ov, int budget_per_cu, BaWidePlan* p, PerCu per_cu, Allow allow, Admit admit) {
  if (p->form != BA_FORM_MULTI || ov.lm_wave_chunks > 0) return false;
  const int per_cu0 = per_cu(p->lds);
  int blocks = p->blocks;
  for (int k = p->k + 1; k <= LM_MAX_WAVE_CHUNKS; ++k) {
    if (ba_lm_blocks(s.C, k) == blocks) continue;  // (no workgroup saved)
    blocks = ba_lm_blocks(s.C, k);
    const size_t lds = ba_plan_wide_lds(s, k);
    if (lds > LM_LDS_LIMIT || per_cu0 <= 0) break;
    const int per_cu_k = per_cu(lds);
    if (per_cu_k < per_cu0 || !allow(lds)) break;
    if (admit(ba_plan_cost(blocks, per_cu_k, budget_per_cu))) { p->k = k; p->lds = lds; p->blocks = blocks; return true; }
  }
  return false;
}

#endif  // SVO_BA_PLAN_H_
