// LDS sizes of the bundle adjuster's kernels (csrc/ba.hip): the staging area of an owner set, the dynamic LDS of the wide
// device-resident solve (ba_lm_kernel, ba_lm_grouped_kernel, ba_lm_multi_kernel) and of the compact one (ba_lm_compact_kernel).  The
// kernels carve their LDS by these sizes and the host's launch planning (host/ba_plan.h) allocates by them.  A header of its own,
// free of HIP includes like lm_turns.h, so that tests/sanitize/ba_plan_test.cpp compiles the very text for the host.
#ifndef SVO_LM_LDS_H_
#define SVO_LM_LDS_H_
#include <stddef.h>

#include "lm_turns.h"

constexpr int REC_STRIDE = 38;        // doubles per lane of the staging rows (36 used; even: 16-byte alignment)
constexpr int LMS_STRIDE = 4;         // pass B: four scalars per landmark of a chunk, in the (idle) staging rows
constexpr int LMS_COL = 36;           // pass A: cost and g_p^2 of the landmark of rank r in the spare columns 36, 37 of row r
constexpr int PST_MAX = 2048;         // wire elements a wavefront stages in LDS before it posts them (larger E: posted one by one)
// LDS of an owner set (doubles): the staging rows (their two spare columns carry pass A's landmark scalars; pass B, which does
// not stage, keeps its four scalars per landmark in the rows themselves) | the E partials of the chunk on their way out
// (consecutive threads then post consecutive granules: whole lines) | 4 ints
SVO_LM_HD static inline int wg_lds_doubles(int E) { return 64 * REC_STRIDE + (E <= PST_MAX ? ((E + 1) & ~1) : 0) + 2; }
constexpr int TAB_LDS_WORDS = 1024;   // u16 words of a chunk table ba_lm_kernel keeps in LDS (larger tables: host-driven path)

// controller workspace (doubles) — it lives in the LDS of the staging rows (a pass and a controller turn never overlap):
// payload image, 4 vectors of n, term scratch, U staging
SVO_LM_HD static inline size_t ba_lm_ctl_doubles(int n, int K) { return (size_t)n * n + 3 * (size_t)n + 2 + 4 * (size_t)(n > 0 ? n : 1) + (size_t)(n > 0 ? n : 1) + 14 * (size_t)K + 21 * (size_t)(K > 1 ? K - 1 : 1) + 8; }
// dynamic LDS of ba_lm_kernel (doubles): [staging rows + landmark scalars of CPW wavefronts | controller workspace] (union) |
// chunk tables | Jacobi scales of the pose columns | step block [dc | candidate poses | current poses]
// A workgroup is LM_CPW wavefronts; each takes `kw` chunks in turn (ba_lm_multi_kernel; kw = 1: ba_lm_kernel, one chunk per wavefront).
// (LM_CPW, LM_MAX_WAVE_CHUNKS, ba_lm_blocks: lm_turns.h)
SVO_LM_HD static inline int ba_wire_elements(int K) { const int F = K - 1; return 18 * F * (F + 1) + 33 * F + 2; }
SVO_LM_HD static inline size_t ba_lm_union_doubles(int n, int K) { const size_t a = (size_t)LM_CPW * (size_t)wg_lds_doubles(ba_wire_elements(K)), b = ba_lm_ctl_doubles(n, K); return a > b ? a : b; }
SVO_LM_HD static inline size_t ba_lm_lds_doubles(int n, int K, int tab_words /* per chunk, a multiple of 4, <= TAB_LDS_WORDS */, int kw = 1) {
  // behind the union and the kw tables of every wavefront: Jacobi scales (nn) | spare (nn) | step block [dc (nn) | candidate poses (7 K) | current poses (7 K)] — the kernel's
  // carve-up (cSc, sStep).  (Until the end of round 4 this said 2 nn: the current poses' tail lay nn doubles beyond the allocation, inside the
  // allocation granule for the 5-keyframe window and outside it from n = 36 on — NaN poses, found when larger windows first took this kernel.)
  return ba_lm_union_doubles(n, K) + (size_t)LM_CPW * (size_t)kw * (size_t)tab_words / 4 + 3 * (size_t)(n > 0 ? n : 1) + 14 * (size_t)K;
}

// the compact form: a solve is NW <= LMC_MAX_WAVES wavefronts in one workgroup, each with ONE staging area
constexpr int LMC_MAX_WAVES = 6;
SVO_LM_HD static inline int lmc_wave_doubles(int E) { return 64 * REC_STRIDE + ((E + 1) & ~1) + 2 + 4; }  // rows | partials | 4 ints | pass B's four sums
SVO_LM_HD static inline size_t ba_lmc_union_doubles(int n, int K, int NW) {
  const size_t a = (size_t)NW * (size_t)lmc_wave_doubles(ba_wire_elements(K)), b = ba_lm_ctl_doubles(n, K);
  return a > b ? a : b;
}
// dynamic LDS (doubles): [NW wave areas | controller workspace] (union) | NW chunk tables | running totals (E) | running group sums (E) |
// pass B's totals and group sums (4 + 4) | Jacobi scales of the pose columns (nn) | spare (nn) | step block [dc (nn) | candidate poses (7 K) | current poses (7 K)]
SVO_LM_HD static inline size_t ba_lmc_lds_doubles(int n, int K, int tab_words, int NW) {
  const size_t Ep = ((size_t)ba_wire_elements(K) + 1) & ~(size_t)1, nn = n > 0 ? n : 1;
  return ba_lmc_union_doubles(n, K, NW) + (size_t)NW * (size_t)tab_words / 4 + 2 * Ep + 8 + 3 * nn + 14 * (size_t)K;
}

#endif  // SVO_LM_LDS_H_
