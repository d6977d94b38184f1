// csrc/lm_turns.h compiled for the host: the chunk turns of the wide window solve (ba_lm_multi_kernel) cover every chunk of a solve
// exactly once, for every chunk count, every k the admission can choose and both chunk -> wavefront orders; a wavefront never takes
// more than k turns (it has k chunk tables in LDS); the workgroup count falls monotonically with k.
#include <cstdio>
#include <vector>

#include "lm_turns.h"

int main() {
  long checked = 0;
  // up to 300 chunks: beyond the 288 of the grouped form and the 250 the GPU tests reach
  for (int C = 1; C <= 300; ++C) {
    int prev_blocks = 1 << 30;
    for (int k = 1; k <= LM_MAX_WAVE_CHUNKS; ++k) {
      const int nb = ba_lm_blocks(C, k);
      if (nb < 1 || nb > prev_blocks) { fprintf(stderr, "C %d k %d: %d workgroups after %d\n", C, k, nb, prev_blocks); return 1; }
      if ((long)nb * LM_CPW * k < C || (long)(nb - 1) * LM_CPW * k >= C) { fprintf(stderr, "C %d k %d: %d workgroups do not fit\n", C, k, nb); return 1; }
      prev_blocks = nb;
      for (int contig = 0; contig < 2; ++contig) {
        std::vector<int> taken((size_t)C, 0);
        for (int b = 0; b < nb; ++b)
          for (int w = 0; w < LM_CPW; ++w) {
            const LmTurns T = lm_turns_of(C, k, nb, b, w, contig != 0);
            if (T.count < 0 || T.count > k || T.stride < 1) { fprintf(stderr, "C %d k %d wg %d wave %d: count %d stride %d\n", C, k, b, w, T.count, T.stride); return 1; }
            for (int t = 0; t < T.count; ++t) {
              const int c = T.chunk(t);
              if (c < 0 || c >= C) { fprintf(stderr, "C %d k %d wg %d wave %d turn %d: chunk %d\n", C, k, b, w, t, c); return 1; }
              ++taken[(size_t)c];
            }
            // fewer than k turns only where the next one would lie beyond the problem
            if (T.count < k && T.first < C && T.first + T.count * T.stride < C) {
              fprintf(stderr, "C %d k %d wg %d wave %d: stops at %d turns with chunk %d left\n", C, k, b, w, T.count, T.first + T.count * T.stride);
              return 1;
            }
            ++checked;
          }
        for (int c = 0; c < C; ++c)
          if (taken[(size_t)c] != 1) { fprintf(stderr, "C %d k %d order %d: chunk %d taken %d times\n", C, k, contig, c, taken[(size_t)c]); return 1; }
      }
    }
  }
  printf("lm turns ok %ld\n", checked);
  return 0;
}
