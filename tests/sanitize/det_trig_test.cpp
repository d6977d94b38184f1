// The pose conversions of the keyframe chain (stereo_vo_amd/host/det_trig.h) at their branches, on the host, under ASan + UBSan.
// Reads a file of inputs and prints the bytes of every result; tests/test_host_sanitizers.py compares them with the restatements
// in tests/pipeline_ref.py and tests/pnp_ref.py.
//   input   int32 n_rvec, int32 n_mat, n_rvec x double[3], n_mat x float[9] (row-major)
//   output  per rvec one line "v <R9 of svo_det_rodrigues_f((float) rvec)> <wxyz of svo_det_quat_from_R(R9)> <wxyz of
//           svo_det_quat_from_rvec(rvec)> <svo_det_rvec_from_quat of it> <svo_det_rvec_from_quat of its negative>",
//           per matrix one line "m <wxyz of svo_det_quat_from_R>", every number as the hex digits of its bit pattern
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "det_trig.h"

static void put_f(const float* v, int n) {
  for (int i = 0; i < n; ++i) {
    uint32_t b;
    memcpy(&b, &v[i], sizeof b);
    printf(" %08x", (unsigned)b);
  }
}

static void put_d(const double* v, int n) {
  for (int i = 0; i < n; ++i) {
    uint64_t b;
    memcpy(&b, &v[i], sizeof b);
    printf(" %016llx", (unsigned long long)b);
  }
}

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: det_trig_test <inputs>\n"); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  int32_t n[2] = {0, 0};
  if (fread(n, sizeof(int32_t), 2, f) != 2 || n[0] < 0 || n[1] < 0 || n[0] > (1 << 20) || n[1] > (1 << 20)) { fclose(f); fprintf(stderr, "bad header\n"); return 2; }
  std::vector<double> rv(3 * (size_t)n[0]);
  std::vector<float> mats(9 * (size_t)n[1]);
  const bool ok = fread(rv.data(), sizeof(double), rv.size(), f) == rv.size() && fread(mats.data(), sizeof(float), mats.size(), f) == mats.size();
  fclose(f);
  if (!ok) { fprintf(stderr, "short file\n"); return 2; }
  for (int i = 0; i < n[0]; ++i) {
    const double* r = &rv[3 * (size_t)i];
    const float rf[3] = {(float)r[0], (float)r[1], (float)r[2]};
    float R9[9], qf[4];
    double q[4], nq[4], back[3], nback[3];
    svo_det_rodrigues_f(rf, R9);
    svo_det_quat_from_R(R9, qf);
    svo_det_quat_from_rvec(r, q);
    svo_det_rvec_from_quat(q, back);
    for (int k = 0; k < 4; ++k) nq[k] = -q[k];
    svo_det_rvec_from_quat(nq, nback);
    printf("v");
    put_f(R9, 9); put_f(qf, 4); put_d(q, 4); put_d(back, 3); put_d(nback, 3);
    printf("\n");
  }
  for (int i = 0; i < n[1]; ++i) {
    float qf[4];
    svo_det_quat_from_R(&mats[9 * (size_t)i], qf);
    printf("m");
    put_f(qf, 4);
    printf("\n");
  }
  printf("det trig ok\n");
  return 0;
}
