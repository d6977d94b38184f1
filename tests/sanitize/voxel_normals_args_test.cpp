// The voxel map normals' and the plane align's GPU-free logic (stereo_vo_amd/host/voxel_normals.h, voxel_align_plane.h) walked on the
// host, under ASan + UBSan: every refusal at its boundary with its code, its exact message and its place in the order, the defaults and
// the side array's size, the integer moments and the Jacobi on neighbourhoods whose records the Python restatement gave bit for bit,
// on random neighbourhoods (V orthonormal, V^T C V diagonal) and on degenerate ones (one point, a line, an exact plane, the largest
// magnitudes), H and g from 40 words, a match's terms against a long double restatement, and a few thousand loop steps on words
// summed on the CPU from three synthetic planes.
#include <limits.h>
#include <stdio.h>
#include <string.h>

#include <limits>
#include <random>
#include <vector>

#include "voxel_align_plane.h"
#include "voxel_normals.h"

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { ++fails; fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

static void expect(int rc, const char* err, const char* want, const char* where) {
  if (want) CHECK(rc == SVO_ERR_INVALID && err && strcmp(err, want) == 0, "%s: rc %d, message '%s', wanted '%s'", where, rc, err ? err : "(none)", want);
  else CHECK(rc == SVO_OK && err == nullptr, "%s: rc %d, message '%s', wanted acceptance", where, rc, err ? err : "(none)");
}
#define EXPECT(call, want, where) do { const char* err = nullptr; const int rc_ = (call); expect(rc_, err, want, where); } while (0)

static const float NaNf = std::numeric_limits<float>::quiet_NaN(), Inff = std::numeric_limits<float>::infinity();

static void checks() {
  const char* mc = "voxel_map_normals: min_count must be at least 1";
  const char* mn = "voxel_map_normals: min_neighbours outside 3..27";
  const char* cu = "voxel_map_normals: max_curvature must be finite and in (0, 1]";
  const struct { svo_voxel_normals_params p; const char* want; } cases[] = {
      {{1, 5, 1.0f}, nullptr}, {{0, 5, 1.0f}, mc}, {{-1, 5, 1.0f}, mc}, {{INT_MAX, 5, 1.0f}, nullptr},
      {{1, 2, 1.0f}, mn}, {{1, 3, 1.0f}, nullptr}, {{1, 27, 1.0f}, nullptr}, {{1, 28, 1.0f}, mn}, {{1, INT_MIN, 1.0f}, mn},
      {{1, 5, 0.0f}, cu}, {{1, 5, -0.0f}, cu}, {{1, 5, FLT_MIN}, nullptr}, {{1, 5, nextafterf(1.0f, 2.0f)}, cu}, {{1, 5, -1.0f}, cu},
      {{1, 5, NaNf}, cu}, {{1, 5, Inff}, cu}, {{1, 5, 0.05f}, nullptr},
      {{0, 2, 0.0f}, mc}, {{1, 2, 0.0f}, mn}, {{1, 3, 0.0f}, cu}};  // the order: the first bad field is the one named
  for (const auto& c : cases) EXPECT(voxel_normals_params_check(&c.p, &err), c.want, "params");
  EXPECT(voxel_normals_params_check(nullptr, &err), "voxel_map_normals: null params", "null params");
  alignas(16) static unsigned char buf[64];
  const svo_voxel_normals_params good = {1, 5, 1.0f}, bad = {0, 5, 1.0f};
  EXPECT(voxel_normals_check(&good, buf, buf + 8, true, &err), nullptr, "ok");
  EXPECT(voxel_normals_check(&good, buf + 16, nullptr, true, &err), nullptr, "no counts");
  EXPECT(voxel_normals_check(nullptr, nullptr, buf + 1, true, &err), "voxel_map_normals: null params", "order: params");
  EXPECT(voxel_normals_check(&bad, nullptr, buf + 1, true, &err), mc, "order: bad params");
  EXPECT(voxel_normals_check(&good, nullptr, buf + 1, true, &err), "voxel_map_normals: null normals", "order: null normals");
  for (int off = 1; off < 16; ++off)
    EXPECT(voxel_normals_check(&good, buf + off, buf + 1, true, &err), "voxel_map_normals: normals must be 16-byte aligned", "normals alignment");
  for (int off = 1; off < 8; ++off)
    EXPECT(voxel_normals_check(&good, buf, buf + off, true, &err), "voxel_map_normals: counts must be 8-byte aligned", "counts alignment");
  EXPECT(voxel_normals_check(&good, buf + 3, buf + 5, false, &err), nullptr, "host pointers of any alignment");
  EXPECT(voxel_normals_check(&good, nullptr, nullptr, false, &err), "voxel_map_normals: null normals", "host null normals");
  svo_voxel_normals_params d = {7, 7, 7.0f};
  CHECK(voxel_normals_default_params(&d) == SVO_OK && d.min_count == 1 && d.min_neighbours == 5 && d.max_curvature == 1.0f, "defaults");
  CHECK(voxel_normals_default_params(nullptr) == SVO_ERR_INVALID, "defaults null");
  EXPECT(voxel_normals_params_check(&d, &err), nullptr, "the defaults pass");
  size_t bytes = 1;
  svo_voxel_map_params mp = {0.1f, 8, 0.0f};
  CHECK(voxel_normals_bytes(&mp, &bytes) == SVO_OK && bytes == 4096, "bytes at 2^8");
  mp.capacity_log2 = 28;
  CHECK(voxel_normals_bytes(&mp, &bytes) == SVO_OK && bytes == ((size_t)16 << 28), "bytes at 2^28");
  mp.capacity_log2 = 29;
  CHECK(voxel_normals_bytes(&mp, &bytes) == SVO_ERR_INVALID && bytes == 0, "bytes refused");
  CHECK(voxel_normals_bytes(&mp, nullptr) == SVO_ERR_INVALID && voxel_normals_bytes(nullptr, &bytes) == SVO_ERR_INVALID, "bytes null");
  const size_t run = (size_t)VOXEL_THREADS * VOXEL_NORMALS_RUN;  // slots per workgroup
  CHECK(voxel_normals_groups(256) == 1 && voxel_normals_groups(run) == 1 && voxel_normals_groups(run + 1) == 2 && voxel_normals_groups((size_t)1 << 28) == ((size_t)1 << 28) / run, "groups");
  // the plane form: the normals' two checks stand in front of the align's list
  const double m[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  const svo_voxel_align_params ap = {1, 1, 0.2f, 10, 64, 0.001f, 1e-5f};
  svo_voxel_align_result res;
  double q[7] = {1, 0, 0, 0, 0, 0, 0};
  EXPECT(voxel_align_plane_sums_check(buf, buf, 5, m, &ap, buf + 8, &err), nullptr, "plane sums ok");
  EXPECT(voxel_align_plane_sums_check(nullptr, nullptr, -1, nullptr, nullptr, nullptr, &err), "voxel_map_align_plane: null normals", "plane: null normals first");
  for (int off = 1; off < 16; ++off)
    EXPECT(voxel_align_plane_sums_check(buf + off, nullptr, -1, nullptr, nullptr, nullptr, &err), "voxel_map_align_plane: normals must be 16-byte aligned", "plane: alignment second");
  EXPECT(voxel_align_plane_sums_check(buf, nullptr, -1, nullptr, nullptr, nullptr, &err), "voxel_map_align: n must not be negative", "plane: then the align's list");
  EXPECT(voxel_align_plane_sums_check(buf, nullptr, 5, m, &ap, buf + 4, &err), "voxel_map_align: sums must be 8-byte aligned", "plane: sums alignment");
  EXPECT(voxel_align_plane_loop_check(nullptr, nullptr, -1, nullptr, nullptr, nullptr, nullptr, &err), "voxel_map_align_plane: null normals", "plane loop: null normals first");
  EXPECT(voxel_align_plane_loop_check(buf, buf, 5, q, &ap, nullptr, &res, &err), "voxel_map_align: null pose7_out", "plane loop: the align's list");
  EXPECT(voxel_align_plane_loop_check(buf, buf, 5, q, &ap, q, &res, &err), nullptr, "plane loop ok");
}

// ----------------------------------------------------------------------------- the moments and the Jacobi
struct Part { int i, j, l; unsigned count; unsigned long long sx, sy, sz; };
struct Golden { Part parts[17]; int n; float max_curvature; int verdict; unsigned bits[4]; };
// neighbourhoods with the records tests/voxel_normals_ref.py (record_py, min_neighbours 3) gives for them, as bit patterns
static const Golden GOLDEN[] = {
  {{{-1, -1, 0, 1u, 32768ull, 32768ull, 32768ull}, {0, -1, 0, 1u, 32768ull, 32768ull, 32768ull}, {1, -1, 0, 1u, 32768ull, 32768ull, 32768ull}, {-1, 0, 0, 1u, 32768ull, 32768ull, 32768ull}, {0, 0, 0, 1u, 32768ull, 32768ull, 32768ull}, {1, 0, 0, 1u, 32768ull, 32768ull, 32768ull}, {-1, 1, 0, 1u, 32768ull, 32768ull, 32768ull}, {0, 1, 0, 1u, 32768ull, 32768ull, 32768ull}, {1, 1, 0, 1u, 32768ull, 32768ull, 32768ull}}, 9, 1.0f, 0, {0x00000000u, 0x00000000u, 0x3f800000u, 0x00000000u}},
  {{{-1, 1, -1, 8u, 406825ull, 494590ull, 130575ull}, {-1, -1, 0, 8u, 455315ull, 129275ull, 199626ull}, {0, -1, 0, 4u, 3437ull, 191675ull, 56814ull}, {1, -1, 0, 3u, 102088ull, 41839ull, 18856ull}, {-1, 0, 0, 8u, 66426ull, 69332ull, 930ull}, {0, 0, 0, 1u, 27453ull, 28243ull, 21739ull}, {-1, 1, 0, 4u, 141354ull, 229669ull, 177689ull}, {1, 1, 0, 4u, 253379ull, 252994ull, 234289ull}, {-1, -1, 1, 1u, 47341ull, 54382ull, 21752ull}, {1, -1, 1, 6u, 157998ull, 316203ull, 307306ull}, {-1, 0, 1, 6u, 34614ull, 162507ull, 186306ull}, {1, 0, 1, 6u, 96874ull, 252297ull, 247746ull}, {0, 1, 1, 1u, 46877ull, 52991ull, 2368ull}, {1, 1, 1, 7u, 191986ull, 197323ull, 303310ull}}, 14, 1.0f, 0, {0xbef58dd2u, 0x3da6c43du, 0x3f5faaf2u, 0x3e30de34u}},
  {{{-1, 1, -1, 8u, 406825ull, 494590ull, 130575ull}, {-1, -1, 0, 8u, 455315ull, 129275ull, 199626ull}, {0, -1, 0, 4u, 3437ull, 191675ull, 56814ull}, {1, -1, 0, 3u, 102088ull, 41839ull, 18856ull}, {-1, 0, 0, 8u, 66426ull, 69332ull, 930ull}, {0, 0, 0, 1u, 27453ull, 28243ull, 21739ull}, {-1, 1, 0, 4u, 141354ull, 229669ull, 177689ull}, {1, 1, 0, 4u, 253379ull, 252994ull, 234289ull}, {-1, -1, 1, 1u, 47341ull, 54382ull, 21752ull}, {1, -1, 1, 6u, 157998ull, 316203ull, 307306ull}, {-1, 0, 1, 6u, 34614ull, 162507ull, 186306ull}, {1, 0, 1, 6u, 96874ull, 252297ull, 247746ull}, {0, 1, 1, 1u, 46877ull, 52991ull, 2368ull}, {1, 1, 1, 7u, 191986ull, 197323ull, 303310ull}}, 14, 0.05000000074505806f, 3, {0x00000000u, 0x00000000u, 0x00000000u, 0xbf800000u}},
  {{{0, -1, -1, 3u, 163502ull, 51516ull, 31200ull}, {1, 0, -1, 6u, 275094ull, 131540ull, 242666ull}, {-1, 1, -1, 6u, 155117ull, 19205ull, 227004ull}, {1, 1, -1, 6u, 268896ull, 320249ull, 190120ull}, {0, -1, 0, 9u, 96545ull, 327627ull, 332188ull}, {1, -1, 0, 2u, 82156ull, 19512ull, 94520ull}, {0, 0, 0, 3u, 188777ull, 12727ull, 21222ull}, {-1, 1, 0, 7u, 16686ull, 124432ull, 388265ull}, {0, 1, 0, 5u, 238899ull, 221122ull, 76351ull}, {1, 1, 0, 1u, 64692ull, 43802ull, 27139ull}, {-1, -1, 1, 3u, 165255ull, 108481ull, 27952ull}, {0, -1, 1, 6u, 78247ull, 30812ull, 220539ull}, {1, -1, 1, 8u, 483395ull, 523920ull, 325269ull}, {1, 0, 1, 8u, 361150ull, 382470ull, 166567ull}, {-1, 1, 1, 5u, 246457ull, 211701ull, 76811ull}, {0, 1, 1, 9u, 188110ull, 523577ull, 354920ull}, {1, 1, 1, 8u, 142768ull, 270102ull, 410003ull}}, 17, 1.0f, 0, {0x3e93b823u, 0xbd8dcd88u, 0x3f7478d6u, 0x3e84b688u}},
  {{{-1, -1, -1, 9u, 378878ull, 66174ull, 372977ull}, {0, 0, -1, 5u, 254638ull, 138862ull, 154063ull}, {-1, 1, -1, 3u, 152216ull, 3035ull, 124335ull}, {0, 1, -1, 5u, 170868ull, 143489ull, 242713ull}, {1, 1, -1, 9u, 373891ull, 364783ull, 287179ull}, {-1, 0, 0, 3u, 180443ull, 117908ull, 95492ull}, {0, 0, 0, 9u, 148749ull, 555053ull, 174244ull}, {1, 0, 0, 6u, 250210ull, 148299ull, 362506ull}, {-1, 1, 0, 7u, 90086ull, 323370ull, 409139ull}, {1, 1, 0, 7u, 158684ull, 327017ull, 290040ull}, {-1, 0, 1, 3u, 153733ull, 115623ull, 163596ull}, {1, 0, 1, 3u, 165377ull, 188340ull, 10973ull}, {1, 1, 1, 3u, 29053ull, 83191ull, 47591ull}}, 13, 1.0f, 0, {0xbeb6b69bu, 0x3f5cba42u, 0xbeb80ec0u, 0x3e62ab4eu}},
  {{{-1, -1, -1, 2u, 1000ull, 2000ull, 3000ull}, {0, 0, 0, 2u, 1000ull, 2000ull, 3000ull}, {1, 1, 1, 2u, 1000ull, 2000ull, 3000ull}}, 3, 1.0f, 2, {0x00000000u, 0x00000000u, 0x00000000u, 0xbf800000u}},
};

static VoxelMoments moments_of(const Part* p, int n) {
  VoxelMoments m;
  voxel_moments_clear(m);
  for (int i = 0; i < n; ++i) voxel_moments_add(m, p[i].i, p[i].j, p[i].l, p[i].count, p[i].sx, p[i].sy, p[i].sz);
  return m;
}

static void golden() {
  for (const Golden& g : GOLDEN) {
    const VoxelMoments m = moments_of(g.parts, g.n);
    svo_voxel_normal out;
    const int verdict = voxel_normal_finish(m, 3, g.max_curvature, &out);
    unsigned b[4];
    memcpy(b, &out, sizeof(b));
    CHECK(verdict == g.verdict && memcmp(b, g.bits, sizeof(b)) == 0, "golden: verdict %d (%d), record %08x %08x %08x %08x, wanted %08x %08x %08x %08x", verdict,
          g.verdict, b[0], b[1], b[2], b[3], g.bits[0], g.bits[1], g.bits[2], g.bits[3]);
    CHECK(voxel_normal_finish(m, g.n + 1, g.max_curvature, &out) == VOXEL_NORMAL_FEW && out.nx == 0.0f && out.ny == 0.0f && out.nz == 0.0f && out.curvature == -1.0f, "few");
  }
}

static void jacobi_random() {
  std::mt19937_64 rng(7);
  double worst_off = 0.0, worst_orth = 0.0;
  for (int t = 0; t < 20000; ++t) {
    Part parts[27];
    int n = 0;
    for (int c = 0; c < 27; ++c) {
      if (c != 13 && rng() % 3 == 0) continue;
      const unsigned count = 1u + (unsigned)(rng() % (t % 2 ? 9u : 16777215u));
      Part p = {c % 3 - 1, c / 3 % 3 - 1, c / 9 - 1, count, rng() % (65536ull * count), rng() % (65536ull * count), rng() % (65536ull * count)};
      if (t % 7 == 0) { p.sx = 65535ull * count; p.sy = p.sx; p.sz = 0; }  // the ends of the fraction's range
      parts[n++] = p;
    }
    const VoxelMoments m = moments_of(parts, n);
    long long C[6];
    voxel_moments_cov(m, C);
    CHECK(C[0] >= 0 && C[3] >= 0 && C[5] >= 0, "a covariance's diagonal is not negative");
    double l[3], V[9];
    voxel_jacobi(C, l, V);
    const double A[3][3] = {{(double)C[0], (double)C[1], (double)C[2]}, {(double)C[1], (double)C[3], (double)C[4]}, {(double)C[2], (double)C[4], (double)C[5]}};
    const double scale = A[0][0] + A[1][1] + A[2][2] + 1.0;
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        double vtv = 0.0, vav = 0.0;
        for (int k = 0; k < 3; ++k) {
          vtv += V[3 * k + i] * V[3 * k + j];
          for (int q = 0; q < 3; ++q) vav += V[3 * k + i] * A[k][q] * V[3 * q + j];
        }
        const double orth = fabs(vtv - (i == j ? 1.0 : 0.0)), off = fabs(vav - (i == j ? l[i] : 0.0)) / scale;
        worst_orth = orth > worst_orth ? orth : worst_orth;
        worst_off = off > worst_off ? off : worst_off;
      }
    svo_voxel_normal out;
    const int verdict = voxel_normal_finish(m, 3, 1.0f, &out);
    if (verdict == VOXEL_NORMAL_VALID) {
      const double len = sqrt((double)out.nx * out.nx + (double)out.ny * out.ny + (double)out.nz * out.nz);
      const float big = fmaxf(fabsf(out.nx), fmaxf(fabsf(out.ny), fabsf(out.nz)));
      CHECK(fabs(len - 1.0) < 1e-6 && out.curvature >= 0.0f && out.curvature <= 0.3333334f, "a valid record: |n| = %.9f, curvature %.9f", len, out.curvature);
      CHECK(out.nx == big || out.ny == big || out.nz == big, "the sign rule: the largest component is positive");
    } else {
      CHECK(out.nx == 0.0f && out.ny == 0.0f && out.nz == 0.0f && out.curvature == -1.0f, "an invalid record");
    }
  }
  CHECK(worst_orth < 1e-14 && worst_off < 1e-14, "Jacobi after 4 sweeps: orthonormality %.3g, V^T C V - diag %.3g of the trace", worst_orth, worst_off);
}

static void jacobi_degenerate() {
  svo_voxel_normal out;
  // one point 27 times over: C = 0, no rotation, collinear
  Part same[27];
  for (int c = 0; c < 27; ++c) same[c] = {0, 0, 0, 3u, 3000ull, 6000ull, 9000ull};
  long long C[6];
  voxel_moments_cov(moments_of(same, 27), C);
  for (int i = 0; i < 6; ++i) CHECK(C[i] == 0, "equal points have no covariance");
  CHECK(voxel_normal_finish(moments_of(same, 27), 3, 1.0f, &out) == VOXEL_NORMAL_COLLINEAR, "one point is collinear");
  // a line along x: the largest entries the bounds allow on one axis
  Part line[3] = {{-1, 0, 0, 1u, 0ull, 7ull, 9ull}, {0, 0, 0, 1u, 0ull, 7ull, 9ull}, {1, 0, 0, 1u, 65535ull, 7ull, 9ull}};
  CHECK(voxel_normal_finish(moments_of(line, 3), 3, 1.0f, &out) == VOXEL_NORMAL_COLLINEAR && out.curvature == -1.0f, "a line is collinear");
  // exact planes along each axis: the normal is that axis, the curvature 0
  for (int axis = 0; axis < 3; ++axis) {
    Part pl[9];
    int n = 0;
    for (int a = -1; a <= 1; ++a)
      for (int b = -1; b <= 1; ++b) {
        const int o[3] = {axis == 0 ? 0 : a, axis == 1 ? 0 : (axis == 0 ? a : b), axis == 2 ? 0 : b};
        pl[n++] = {o[0], o[1], o[2], 4u, 4ull * 16384, 4ull * 16384, 4ull * 16384};
      }
    CHECK(voxel_normal_finish(moments_of(pl, 9), 5, 0.001f, &out) == VOXEL_NORMAL_VALID, "an exact plane is valid");
    const float want[3] = {axis == 0 ? 1.0f : 0.0f, axis == 1 ? 1.0f : 0.0f, axis == 2 ? 1.0f : 0.0f};
    CHECK(out.nx == want[0] && out.ny == want[1] && out.nz == want[2] && out.curvature == 0.0f, "axis %d: %g %g %g %g", axis, out.nx, out.ny, out.nz, out.curvature);
  }
  // the curvature test holds at equality: lambda = (4, 4, 8) k, curvature exactly 0.25
  Part eq[9] = {{0, 0, 0, 1u, 5ull, 5ull, 5ull}, {1, 0, 1, 1u, 5ull, 5ull, 5ull}, {1, 0, -1, 1u, 5ull, 5ull, 5ull}, {-1, 0, 1, 1u, 5ull, 5ull, 5ull}, {-1, 0, -1, 1u, 5ull, 5ull, 5ull},
                {0, 1, 1, 1u, 5ull, 5ull, 5ull}, {0, 1, -1, 1u, 5ull, 5ull, 5ull}, {0, -1, 1, 1u, 5ull, 5ull, 5ull}, {0, -1, -1, 1u, 5ull, 5ull, 5ull}};
  CHECK(voxel_normal_finish(moments_of(eq, 9), 5, 0.25f, &out) == VOXEL_NORMAL_VALID && out.nx == 1.0f && out.ny == 0.0f && out.nz == 0.0f && out.curvature == 0.25f,
        "equality is valid, ties go to the lowest index: %g %g %g %g", out.nx, out.ny, out.nz, out.curvature);
  CHECK(voxel_normal_finish(moments_of(eq, 9), 5, nextafterf(0.25f, 0.0f), &out) == VOXEL_NORMAL_CURVED, "the float below refuses it");
  // a matrix whose th * th overflows: t = 0 and nothing is a NaN
  const long long huge[6] = {0, 1, 0, 1ll << 62, 0, 5};
  double l[3], V[9];
  voxel_jacobi(huge, l, V);
  for (int i = 0; i < 3; ++i) CHECK(l[i] == l[i], "lambda %d is a NaN", i);
  for (int i = 0; i < 9; ++i) CHECK(V[i] == V[i], "V %d is a NaN", i);
}

// ----------------------------------------------------------------------------- the plane form
static void plane_words() {
  bool seen[22] = {false};
  for (int i = 0; i < 6; ++i)
    for (int k = i; k < 6; ++k) {
      const int w = voxel_align_plane_word(i, k);
      CHECK(w >= 1 && w <= 21 && !seen[w], "word(%d, %d) = %d", i, k, w);
      if (w >= 1 && w <= 21) seen[w] = true;
    }
  CHECK(voxel_align_plane_word(0, 0) == 1 && voxel_align_plane_word(0, 5) == 6 && voxel_align_plane_word(1, 1) == 7 && voxel_align_plane_word(5, 5) == 21, "row-major upper triangle");
  CHECK(voxel_align_plane_scale(0, 2) == 1099511627776.0 && voxel_align_plane_scale(2, 3) == 1073741824.0 && voxel_align_plane_scale(3, 5) == 1048576.0, "the three scales");
  int64_t w[VOXEL_ALIGN_PLANE_WORDS];
  for (int i = 0; i < VOXEL_ALIGN_PLANE_WORDS; ++i) w[i] = 1000 + i;
  double H[6][6], g[6];
  voxel_align_plane_normal(w, H, g);
  for (int i = 0; i < 6; ++i)
    for (int k = 0; k < 6; ++k) {
      const int a = i < k ? i : k, b = i < k ? k : i;
      CHECK(H[i][k] == (double)(1000 + voxel_align_plane_word(a, b)) / voxel_align_plane_scale(a, b), "H[%d][%d]", i, k);
    }
  for (int i = 0; i < 3; ++i) CHECK(g[i] == (double)(1022 + i) / 68719476736.0 && g[3 + i] == (double)(1025 + i) / 268435456.0, "g %d", i);
  // a match's terms against a long double restatement, at the largest magnitudes the bounds allow
  std::mt19937_64 rng(11);
  std::uniform_real_distribution<double> un(-1.0, 1.0);
  for (int t = 0; t < 2000; ++t) {
    double nn[3] = {un(rng), un(rng), un(rng)}, e[3] = {4.6 * un(rng), 4.6 * un(rng), 4.6 * un(rng)}, P[3] = {1023.9 * un(rng), 1023.9 * un(rng), 1023.9 * un(rng)};
    const double len = sqrt(nn[0] * nn[0] + nn[1] * nn[1] + nn[2] * nn[2]);
    for (double& c : nn) c = (double)(float)(c / len);
    const double m[12] = {0, 0, 1, 5, 1, 0, 0, 6, 0, 1, 0, 7};  // a rotation: camera z -> world x, x -> y, y -> z
    long long v[VOXEL_ALIGN_PLANE_TERMS];
    voxel_align_plane_terms(nn, e, m, P, v);
    const long double a[3] = {nn[1], nn[2], nn[0]};
    const long double r = (long double)nn[0] * e[0] + (long double)nn[1] * e[1] + (long double)nn[2] * e[2];
    const long double j[6] = {a[0], a[1], a[2], P[1] * a[2] - P[2] * a[1], P[2] * a[0] - P[0] * a[2], P[0] * a[1] - P[1] * a[0]};
    for (int i = 0; i < 6; ++i)
      for (int k = i; k < 6; ++k) {
        const long double want = j[i] * j[k] * voxel_align_plane_scale(i, k);
        CHECK(fabsl((long double)v[voxel_align_plane_word(i, k) - 1] - want) <= 0.5L + fabsl(want) * 1e-15L && fabsl(want) < 8796093022208.0L, "term (%d, %d)", i, k);
      }
    for (int i = 0; i < 6; ++i) {
      const long double want = j[i] * r * (i < 3 ? 68719476736.0L : 268435456.0L);
      CHECK(fabsl((long double)v[21 + i] - want) <= 0.5L + fabsl(want) * 1e-15L && fabsl(want) < 8796093022208.0L, "g term %d", i);
    }
    CHECK(fabsl((long double)v[27] - r * r * 268435456.0L) <= 0.5L + 1e-6L, "the cost");
  }
}

// Words summed on the CPU: points on three planes n . X = d (world = the true camera frame), each matched with its foot on its plane.
struct Scene {
  std::vector<double> P, n;  // 3 doubles each per point
  std::vector<double> d;
};

static void sums_of(const Scene& s, const double* m, int planes, int64_t* w) {
  memset(w, 0, VOXEL_ALIGN_PLANE_WORDS * sizeof(int64_t));
  for (size_t i = 0; i < s.d.size(); ++i) {
    if ((int)(i % 3) >= planes) continue;
    const double* P = &s.P[3 * i];
    const double* n = &s.n[3 * i];
    double wr[3], e[3];
    for (int r = 0; r < 3; ++r) wr[r] = m[4 * r] * P[0] + m[4 * r + 1] * P[1] + m[4 * r + 2] * P[2] + m[4 * r + 3];
    const double dist = n[0] * wr[0] + n[1] * wr[1] + n[2] * wr[2] - s.d[i];
    for (int r = 0; r < 3; ++r) e[r] = dist * n[r];
    long long v[VOXEL_ALIGN_PLANE_TERMS];
    voxel_align_plane_terms(n, e, m, P, v);
    for (int t = 0; t < VOXEL_ALIGN_PLANE_TERMS; ++t) w[1 + t] += v[t];
    w[0] += 1;
    w[29] += 1;
  }
}

static void plane_loop() {
  std::mt19937_64 rng(3);
  std::uniform_real_distribution<double> un(-1.0, 1.0);
  Scene s;
  const double planes[3][4] = {{0.0, 1.0, 0.0, 0.9}, {0.0, 0.0, 1.0, 5.0}, {1.0, 0.0, 0.0, 2.6}};
  for (int i = 0; i < 300; ++i) {
    const double* pl = planes[i % 3];
    double X[3] = {3.0 * un(rng), 3.0 * un(rng), 3.0 + 2.0 * un(rng)};
    const double off = pl[0] * X[0] + pl[1] * X[1] + pl[2] * X[2] - pl[3];
    for (int r = 0; r < 3; ++r) { X[r] -= off * pl[r]; s.P.push_back(X[r]); s.n.push_back(pl[r]); }
    s.d.push_back(pl[3]);
  }
  const svo_voxel_align_params prm = {1, 1, 0.2f, 10, 64, 1e-9f, 1e-9f};
  int steps = 0, converged = 0;
  for (int t = 0; t < 400; ++t) {
    double q[7] = {1.0, 0.01 * un(rng), 0.01 * un(rng), 0.01 * un(rng), 0.05 * un(rng), 0.05 * un(rng), 0.05 * un(rng)}, out[7];
    svo_voxel_align_result res;
    const int rc = voxel_align_plane_loop(q, &prm, [&](const double* m, int64_t* w) { sums_of(s, m, 3, w); return (int)SVO_OK; }, out, &res);
    CHECK(rc == SVO_OK && res.first_matched == 300 && res.last_cost <= res.first_cost, "loop %d: rc %d", t, rc);
    steps += res.iterations;
    converged += res.status == SVO_VOXEL_ALIGN_CONVERGED;
    const double err = fabs(out[1]) + fabs(out[2]) + fabs(out[3]) + fabs(out[4]) + fabs(out[5]) + fabs(out[6]);
    CHECK(err < 1e-6 && fabs(out[0] * out[0] + out[1] * out[1] + out[2] * out[2] + out[3] * out[3] - 1.0) < 1e-15, "loop %d ends %.3g from the truth (status %d after %d)", t, err,
          res.status, res.iterations);
  }
  CHECK(steps >= 1200 && converged == 400, "%d loop steps, %d runs converged", steps, converged);
  // one plane holds three freedoms only: a pivot fails, no step is taken, the input pose comes back bit for bit
  double q[7] = {1.0, 0.001, 0.002, -0.001, 0.01, 0.02, 0.03}, out[7];
  svo_voxel_align_result res;
  CHECK(voxel_align_plane_loop(q, &prm, [&](const double* m, int64_t* w) { sums_of(s, m, 1, w); return (int)SVO_OK; }, out, &res) == SVO_OK, "one plane: rc");
  CHECK(res.status == SVO_VOXEL_ALIGN_DEGENERATE && res.iterations == 1 && memcmp(q, out, sizeof(q)) == 0, "one plane: status %d after %d", res.status, res.iterations);
  // too few contributing matches; an error of the functor ends the loop with nothing written
  svo_voxel_align_params few = prm;
  few.min_matches = 301;
  CHECK(voxel_align_plane_loop(q, &few, [&](const double* m, int64_t* w) { sums_of(s, m, 3, w); return (int)SVO_OK; }, out, &res) == SVO_OK &&
            res.status == SVO_VOXEL_ALIGN_TOO_FEW && res.first_matched == 300 && memcmp(q, out, sizeof(q)) == 0, "too few");
  out[0] = 77.0;
  res.status = 77;
  CHECK(voxel_align_plane_loop(q, &prm, [&](const double*, int64_t*) { return (int)SVO_ERR_HIP; }, out, &res) == SVO_ERR_HIP && out[0] == 77.0 && res.status == 77, "functor error");
}

int main() {
  checks();
  golden();
  jacobi_random();
  jacobi_degenerate();
  plane_words();
  plane_loop();
  if (fails) { fprintf(stderr, "%d failures\n", fails); return 1; }
  printf("voxel normals args ok\n");
  return 0;
}
