// Turn arithmetic of the wide window solve with several chunks per wavefront (ba_lm_multi_kernel): how many workgroups a solve of C
// chunks takes at k chunks per wavefront, and which chunks wavefront `wave` of workgroup `block` takes in turn.  A header of its own,
// free of HIP includes, so that tests/sanitize/lm_turns_test.cpp can compile the kernel's very arithmetic for the host and check
// that every chunk is taken exactly once for every (C, k) the admission can choose.
#ifndef SVO_LM_TURNS_H_
#define SVO_LM_TURNS_H_

#if defined(__HIPCC__)
#define SVO_LM_HD __host__ __device__
#else
#define SVO_LM_HD
#endif

constexpr int LM_CPW = 2;              // wavefronts (chunks in flight) of a workgroup of the wide solve
// Chunks a wavefront may take in turn.  The kernel holds nothing per turn but the chunk's table in LDS (tab_words u16 words), so the
// limit is a bound on the LM chain's length, not on a resource: a solve at k = 8 runs 8 turns per pass on an eighth of the
// workgroups.  The admission (ba_device_lm_launch) raises k above the default only as far as the workgroups per CU stay what they
// are at the default.
constexpr int LM_MAX_WAVE_CHUNKS = 8;

SVO_LM_HD inline int ba_lm_blocks(int C, int kw) { return (C + LM_CPW * kw - 1) / (LM_CPW * kw); }  // workgroups of a wide solve

// The chunks a wavefront takes in turn: first, first + stride, ... (`count` of them lie below C).  Strided (default): slot
// s = 2 x workgroup + wavefront takes s, s + S, s + 2 S, ... with S = 2 x workgroups, so neighbouring chunks — the slow ones (a
// chunk of brand-new landmarks of the newest pose) come in runs — land on different wavefronts; contiguous: the workgroup's own
// 2 kw chunks, alternating between its two wavefronts.
struct LmTurns {
  int first, stride, count;
  SVO_LM_HD int chunk(int t) const { return first + t * stride; }
};
SVO_LM_HD inline LmTurns lm_turns_of(int C, int kw, int n_blocks, int block, int wave, bool contig) {
  LmTurns T;
  if (contig) { T.first = block * LM_CPW * kw + wave; T.stride = LM_CPW; }
  else { T.first = block * LM_CPW + wave; T.stride = LM_CPW * n_blocks; }
  const int left = T.first < C ? (C - 1 - T.first) / T.stride + 1 : 0;
  T.count = left < kw ? left : kw;
  return T;
}

#endif  // SVO_LM_TURNS_H_
