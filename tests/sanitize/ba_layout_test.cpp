// The problem layout of the bundle adjuster (stereo_vo_amd/host/ba_layout.h) — the host half of the declared summation order —
// walked on the host, under ASan + UBSan.  A brute-force restatement walks landmarks, then i, then t >= i, and builds per upper
// pose-pair block the expected list of entries (lane i, lane t, transposed) and per free pose the expected list of lanes; both
// are compared with the tables of plan(), entry for entry and in order.  Also: the chunk boundaries, the dimensions' formulas
// (beyond 128 and beyond 2,048 chunks too), the staging image of write_image(), and every rejection at its boundary.
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "ba_layout.h"

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { ++fails; fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

struct Problem {
  int K = 1, npts = 0;
  std::vector<int32_t> op, oj;
  void landmark(const std::vector<int>& poses) { for (int k : poses) { op.push_back(k); oj.push_back(npts); } ++npts; }  // an empty list: never observed
  int M() const { return (int)op.size(); }
};

struct Entry { int i, t, transposed; };
static bool operator==(const Entry& a, const Entry& b) { return a.i == b.i && a.t == b.t && a.transposed == b.transposed; }

static int plan(BaLayout& l, const Problem& p, int acc = SVO_BA_ACC_AUTO, bool keys = false, const char** why = nullptr) {
  const char* err = nullptr;
  const int rc = l.plan(p.K, p.npts, p.M(), p.op.data(), p.oj.data(), acc, keys, &err);
  CHECK((rc == SVO_OK) == (err == nullptr), "status %d and message %s disagree", rc, err ? err : "(none)");
  if (why) *why = err;
  return rc;
}

// chunks, tables and dimensions of a planned problem against the restatement
static void check_plan(const Problem& p, const BaLayout& l, const char* what) {
  const int K = p.K, F = K - 1, nU = F * (F + 1) / 2, M = p.M();
  CHECK(l.K == K && l.n == 6 * F && l.M == M && l.L == p.npts, "%s: dimensions", what);
  // landmark CSR
  std::vector<int> first(p.npts + 1, 0);
  for (int o = 0; o < M; ++o) first[p.oj[o] + 1]++;
  for (int j = 0; j < p.npts; ++j) first[j + 1] += first[j];
  CHECK((int)l.lm_start.size() == p.npts + 1 && std::equal(first.begin(), first.end(), l.lm_start.begin()), "%s: landmark CSR", what);
  // chunks: whole landmarks, greedily, at most 64 observations
  std::vector<int> chunks{0};
  for (int j = 0, cur = 0; j < p.npts; ++j) {
    const int len = first[j + 1] - first[j];
    if (cur + len > 64) { chunks.push_back(first[j]); cur = 0; }
    cur += len;
  }
  chunks.push_back(M);
  if (M == 0) chunks = {0, 0};
  CHECK(l.C == (int)chunks.size() - 1 && (int)l.chunks.size() == l.C + 1 && std::equal(chunks.begin(), chunks.end(), l.chunks.begin()), "%s: chunks (%d)", what, l.C);
  if (l.C != (int)chunks.size() - 1) return;
  for (int c = 0; c < l.C; ++c) CHECK(chunks[c + 1] - chunks[c] <= 64 && (chunks[c + 1] > chunks[c] || M == 0), "%s: chunk %d holds %d", what, c, chunks[c + 1] - chunks[c]);
  // dimensions
  const int C = l.C, E = 36 * F * (F + 1) / 2 + 33 * F + 2;
  CHECK(l.E == E && l.Epad % 8 == 0 && l.Epad >= E && l.Epad < E + 8, "%s: E %d, Epad %d", what, l.E, l.Epad);
  const int G = C <= 128 ? 1 : (C + 127) / 128;
  const int CPW = ((long long)l.Epad * C * 16 <= (64ll << 20) && C <= 2048) ? 1 : G;
  CHECK(l.G == G && l.CPW == CPW && l.GS == G / CPW && l.NG == (C + CPW - 1) / CPW, "%s: G %d, CPW %d, GS %d, NG %d for %d chunks", what, l.G, l.CPW, l.GS, l.NG, C);
  CHECK(l.det == 1, "%s: not deterministic", what);
  // tables
  CHECK((int)l.tab_off.size() == C + 1 && l.tab_off.back() == l.tab.size(), "%s: table offsets", what);
  int max_words = 0;
  for (int c = 0, j = 0; c < C; ++c) {
    const int c0 = chunks[c], c1 = chunks[c + 1];
    std::vector<std::vector<Entry>> block((size_t)nU);
    std::vector<std::vector<int>> lanes((size_t)F);
    std::vector<int> block_of((size_t)F * F, -1);  // row-major numbering of the upper blocks, by enumeration
    for (int ka = 0, q = 0; ka < F; ++ka) for (int kb = ka; kb < F; ++kb) block_of[ka * F + kb] = q++;
    for (; j < p.npts && first[j] < c1; ++j) {  // the landmarks of this chunk
      if (first[j + 1] == first[j]) continue;
      CHECK(first[j] >= c0, "%s: landmark %d starts before its chunk", what, j);
      CHECK(first[j + 1] <= c1, "%s: landmark %d straddles chunks", what, j);
      for (int i = first[j]; i < first[j + 1]; ++i) {
        const int ki = p.op[i] - 1;
        if (ki < 0) continue;
        lanes[ki].push_back(i - c0);
        for (int t = i; t < first[j + 1]; ++t) {
          const int kt = p.op[t] - 1;
          if (kt < 0) continue;
          if (ki <= kt) block[block_of[ki * F + kt]].push_back({i - c0, t - c0, 0});
          if (t != i && kt <= ki) block[block_of[kt * F + ki]].push_back({i - c0, t - c0, 1});
        }
      }
    }
    const uint32_t w0 = l.tab_off[c], w1 = l.tab_off[c + 1];
    CHECK(w0 % 2 == 0 && w1 % 2 == 0 && w1 > w0, "%s: table %d at u16 offsets %u..%u", what, c, w0, w1);
    max_words = std::max(max_words, (int)(w1 - w0));
    const uint16_t* w = l.tab.data() + w0;
    const uint16_t* ent = w + nU + 1 + F + 1;
    size_t n_ent = 0, n_free = 0;
    for (int q = 0; q < nU; ++q) n_ent += block[q].size();
    for (int k = 0; k < F; ++k) n_free += lanes[k].size();
    const size_t words = (size_t)nU + 1 + F + 1 + n_ent + (n_free + 1) / 2;
    CHECK(w1 - w0 == ((words + 1) & ~(size_t)1), "%s: table %d has %u words, expected %zu", what, c, w1 - w0, words);
    if (w1 - w0 < words) continue;
    const uint8_t* lane = reinterpret_cast<const uint8_t*>(ent + n_ent);
    for (int q = 0, at = 0; q < nU; ++q) {
      CHECK(w[q] == at && w[q + 1] == at + (int)block[q].size(), "%s: chunk %d block %d spans %d..%d, expected %d + %zu", what, c, q, w[q], w[q + 1], at, block[q].size());
      for (size_t e = 0; e < block[q].size() && w[q + 1] == at + (int)block[q].size(); ++e) {
        const uint16_t v = ent[at + e];
        const Entry got = {v & 0x7f, v >> 8, (v >> 7) & 1};
        CHECK(got == block[q][e], "%s: chunk %d block %d entry %zu is (%d, %d, %d), expected (%d, %d, %d)", what, c, q, e, got.i, got.t, got.transposed,
              block[q][e].i, block[q][e].t, block[q][e].transposed);
      }
      at += (int)block[q].size();
    }
    for (int k = 0, at = 0; k < F; ++k) {
      const uint16_t* lo = w + nU + 1;
      CHECK(lo[k] == at && lo[k + 1] == at + (int)lanes[k].size(), "%s: chunk %d pose %d spans %d..%d", what, c, k, lo[k], lo[k + 1]);
      for (size_t e = 0; e < lanes[k].size() && lo[k + 1] == at + (int)lanes[k].size(); ++e)
        CHECK(lane[at + e] == lanes[k][e], "%s: chunk %d pose %d lane %zu is %d, expected %d", what, c, k, e, lane[at + e], lanes[k][e]);
      at += (int)lanes[k].size();
    }
  }
  CHECK(l.tab_max_words == max_words, "%s: tab_max_words %d, the largest table has %d", what, l.tab_max_words, max_words);
  CHECK(l.tab_lds_words() == (max_words <= 4096 ? (max_words + 3) / 4 * 4 : 0), "%s: tab_lds_words", what);
}

// the staging image: records, pixels, tables, keys, points and poses twice; 256-byte aligned pieces that do not overlap
static void check_image(const Problem& p, const BaLayout& l, bool keys, const char* what) {
  const int M = p.M();
  std::vector<double> pts(3 * (size_t)p.npts + 1), poses(7 * (size_t)p.K), uv(2 * (size_t)M + 1);
  std::vector<int64_t> ids((size_t)p.npts + 1);
  for (size_t i = 0; i < pts.size(); ++i) pts[i] = 0.5 + (double)i;
  for (size_t i = 0; i < poses.size(); ++i) poses[i] = -2.0 - (double)i;
  for (size_t i = 0; i < uv.size(); ++i) uv[i] = 1e3 + (double)i;
  for (size_t j = 0; j < ids.size(); ++j) ids[j] = (int64_t)(0x100000000ll * (j % 3) + 7 * j + 1);  // keys are the low 32 bits
  const size_t nslots = (size_t)l.C * 64;
  struct Piece { const char* name; size_t off, bytes; };
  const Piece piece[] = {{"points", l.o_pts, 24 * (size_t)p.npts}, {"candidate points", l.o_cpts, 24 * (size_t)p.npts}, {"records", l.o_rec, 16 * nslots},
                         {"uv", l.o_uv, 16 * nslots}, {"tables", l.o_tab, 2 * l.tab.size()}, {"table offsets", l.o_toff, 4 * l.tab_off.size()},
                         {"keys", l.o_key, keys ? 4 * (size_t)p.npts : 0}, {"poses", l.o_p0, 56 * (size_t)p.K}, {"candidate poses", l.o_p1, 56 * (size_t)p.K}};
  size_t end = 0;
  for (const Piece& q : piece) {
    CHECK(q.off % 256 == 0 && q.off >= end, "%s: %s at %zu, the piece before ends at %zu", what, q.name, q.off, end);
    end = q.off + q.bytes;
  }
  CHECK(l.total >= end && l.total % 256 == 0 && l.image_bytes() >= l.total && l.image_bytes() % 16 == 0 && l.image_bytes() < l.total + 16, "%s: image of %zu bytes, pieces end at %zu", what, l.image_bytes(), end);
  std::vector<uint8_t> h(l.image_bytes(), 0xAB);  // exactly as large as promised: ASan sees a byte too many
  l.write_image(h.data(), p.op.data(), p.oj.data(), pts.data(), poses.data(), uv.data(), keys ? ids.data() : nullptr);
  CHECK(!memcmp(h.data() + l.o_pts, pts.data(), 24 * (size_t)p.npts) && !memcmp(h.data() + l.o_cpts, pts.data(), 24 * (size_t)p.npts), "%s: points", what);
  CHECK(!memcmp(h.data() + l.o_p0, poses.data(), 56 * (size_t)p.K) && !memcmp(h.data() + l.o_p1, poses.data(), 56 * (size_t)p.K), "%s: poses", what);
  CHECK(!memcmp(h.data() + l.o_tab, l.tab.data(), 2 * l.tab.size()) && !memcmp(h.data() + l.o_toff, l.tab_off.data(), 4 * l.tab_off.size()), "%s: tables", what);
  const int32_t* rec = reinterpret_cast<const int32_t*>(h.data() + l.o_rec);
  const double* suv = reinterpret_cast<const double*>(h.data() + l.o_uv);
  std::vector<int> first(p.npts + 1, 0);
  for (int o = 0; o < M; ++o) first[p.oj[o] + 1]++;
  for (int j = 0; j < p.npts; ++j) first[j + 1] += first[j];
  int real = 0;
  for (int c = 0; c < l.C; ++c)
    for (int lane = 0; lane < 64; ++lane) {
      const size_t s = (size_t)c * 64 + lane;
      const int o = l.chunks[c] + lane;
      if (o < l.chunks[c + 1]) {
        const int j = p.oj[o];
        const int32_t want[4] = {p.op[o], j, first[j] - l.chunks[c], first[j + 1] - first[j]};
        CHECK(!memcmp(rec + 4 * s, want, 16), "%s: slot %zu is {%d, %d, %d, %d}, expected {%d, %d, %d, %d}", what, s, rec[4 * s], rec[4 * s + 1], rec[4 * s + 2], rec[4 * s + 3], want[0], want[1], want[2], want[3]);
        CHECK(want[2] >= 0 && want[2] + want[3] <= 64, "%s: slot %zu's segment leaves the chunk", what, s);
        CHECK(suv[2 * s] == uv[2 * (size_t)o] && suv[2 * s + 1] == uv[2 * (size_t)o + 1], "%s: pixel of slot %zu", what, s);
        ++real;
      } else {
        const int32_t want[4] = {-1, 0, lane, 0};
        CHECK(!memcmp(rec + 4 * s, want, 16) && suv[2 * s] == 0.0 && suv[2 * s + 1] == 0.0, "%s: padding slot %zu", what, s);
      }
    }
  CHECK(real == M, "%s: %d real slots for %d observations", what, real, M);
  if (keys) {
    const uint32_t* key = reinterpret_cast<const uint32_t*>(h.data() + l.o_key);
    for (int j = 0; j < p.npts; ++j) CHECK(key[j] == (uint32_t)ids[j], "%s: key %d", what, j);
  }
}

static void check_all(const Problem& p, const char* what, bool image = true) {
  BaLayout l;
  CHECK(plan(l, p) == SVO_OK, "%s: refused", what);
  check_plan(p, l, what);
  if (!image) return;
  check_image(p, l, false, what);
  CHECK(plan(l, p, SVO_BA_ACC_AUTO, true) == SVO_OK, "%s: refused with keys", what);  // the same object again: nothing of the last plan survives
  check_plan(p, l, what);
  check_image(p, l, true, what);
}

static void rejected(BaLayout& l, const Problem& p, const char* msg, const char* what, int acc = SVO_BA_ACC_AUTO) {
  const char* why = nullptr;
  CHECK(plan(l, p, acc, false, &why) == SVO_ERR_INVALID && why && !strcmp(why, msg), "%s: %s", what, why ? why : "accepted");
  CHECK(l.K == 0 && l.M == 0 && l.L == 0 && l.C == 0 && l.n == 0, "%s: a rejected problem is still reported", what);
}

int main() {
  // ---- K = 1, 2, 3, 5, 9: landmark lengths 1..K over rotating pose sets, a landmark seen twice by one pose, one never observed,
  //      one seen by the fixed pose only — enough of them for several chunks
  for (int K : {1, 2, 3, 5, 9}) {
    Problem p;
    p.K = K;
    for (int rep = 0; rep < 14; ++rep) {
      for (int len = 1; len <= K; ++len) {
        std::vector<int> poses;
        for (int a = 0; a < len; ++a) poses.push_back((rep + a * K / len) % K);  // `len` distinct poses
        std::sort(poses.begin(), poses.end());
        p.landmark(poses);
      }
      p.landmark({});
      p.landmark({0});
      if (K > 1) p.landmark({0, rep % (K - 1) + 1, rep % (K - 1) + 1, K - 1});
      p.landmark({0, 0});
    }
    char what[32];
    snprintf(what, sizeof(what), "K = %d", K);
    check_all(p, what);
    BaLayout l;
    plan(l, p);
    CHECK(!l.mfma_ok, "%s: two observations of a landmark in one pose and mfma_ok", what);
    if (K == 1) CHECK(l.E == 2 && l.n == 0, "K = 1: E %d", l.E);
    else CHECK(l.C > 1, "%s: one chunk only", what);
  }
  // ---- a landmark seen twice by one free pose: the direct entry first, then the transposed one
  {
    Problem p;
    p.K = 3;
    p.landmark({1});
    p.landmark({2, 2});
    BaLayout l;
    CHECK(plan(l, p) == SVO_OK && !l.mfma_ok, "seen twice");
    check_plan(p, l, "seen twice");
    const uint16_t* w = l.tab.data();            // F = 2, nU = 3: offsets w[0..3], lane offsets w[4..6], entries from w[7]
    const uint16_t want[4] = {1 | 1 << 8, 1 | 2 << 8, 1 | 0x80 | 2 << 8, 2 | 2 << 8};  // block (1, 1): (1,1) (1,2) (1,2)^T (2,2)
    CHECK(w[2] == 1 && w[3] == 5 && !memcmp(w + 7 + 1, want, sizeof(want)), "seen twice: block (1, 1) is not direct, direct, transposed, direct");
    Problem q;
    q.K = 3;
    q.landmark({1});
    q.landmark({1, 2});
    CHECK(plan(l, q) == SVO_OK && l.mfma_ok, "one observation per (landmark, pose) and n <= 128 is MFMA-eligible");
    CHECK(plan(l, q, SVO_BA_ACC_ATOMICS) == SVO_OK && !l.mfma_ok && !l.det, "atomics: neither deterministic nor MFMA");
    CHECK(plan(l, q, SVO_BA_ACC_MFMA) == SVO_OK && l.mfma_ok && !l.det && l.tab.empty() && l.tab_lds_words() == 0, "MFMA: no tables");
    check_image(q, l, false, "MFMA");
    rejected(l, p, "ba: MFMA accumulation needs <= 22 poses and one observation per (landmark, pose)", "MFMA with a pose seen twice", SVO_BA_ACC_MFMA);
    q.K = 23;  // n = 132
    rejected(l, q, "ba: MFMA accumulation needs <= 22 poses and one observation per (landmark, pose)", "MFMA with 23 poses", SVO_BA_ACC_MFMA);
    q.K = 22;
    CHECK(plan(l, q, SVO_BA_ACC_MFMA) == SVO_OK, "MFMA with 22 poses");
  }
  // ---- chunk boundaries
  {
    BaLayout l;
    Problem p;
    p.K = 2;
    check_all(p, "M = 0, no landmark");
    p.landmark({});
    check_all(p, "M = 0");
    CHECK(plan(l, p) == SVO_OK && l.C == 1 && l.NG == 1 && l.chunks[0] == 0 && l.chunks[1] == 0, "M = 0 is one empty chunk");
    Problem a;
    a.K = 2;
    for (int j = 0; j < 32; ++j) a.landmark({0, 1});
    check_all(a, "64 observations");
    CHECK(plan(l, a) == SVO_OK && l.C == 1, "64 observations are one chunk");
    a.landmark({1});
    check_all(a, "65 observations");
    CHECK(plan(l, a) == SVO_OK && l.C == 2 && l.chunks[1] == 64, "65 observations are two chunks");
    Problem s;
    s.K = 5;
    for (int j = 0; j < 12; ++j) s.landmark({0, 1, 2, 3, 4});
    s.landmark({0, 1, 2, 3, 4});  // 60 + 5 > 64: closes the chunk at 60
    s.landmark({1, 2, 3, 4});     // 5 + 4
    check_all(s, "a landmark that would straddle");
    CHECK(plan(l, s) == SVO_OK && l.C == 2 && l.chunks[1] == 60 && l.chunks[2] == 69, "a straddling landmark closes the chunk early");
    Problem full;
    full.K = 64;
    std::vector<int> all;
    for (int k = 0; k < 64; ++k) all.push_back(k);
    full.landmark({63});
    full.landmark(all);           // 64 observations of one landmark: a chunk of its own
    full.landmark({0});
    check_all(full, "a landmark of 64 observations");
    CHECK(plan(l, full) == SVO_OK && l.C == 3 && l.E == 36 * 63 * 64 / 2 + 33 * 63 + 2, "a landmark of 64 observations");
  }
  // ---- more than 128 chunks: G = 2; more than 2,048: one stored partial per group
  {
    BaLayout l;
    for (int C : {128, 129, 257, 2048, 2049}) {
      Problem p;
      p.K = 2;
      for (int j = 0; j < 64 * C; ++j) p.landmark({j % 3 ? 1 : 0});
      char what[32];
      snprintf(what, sizeof(what), "%d chunks", C);
      check_all(p, what, C <= 257);
      CHECK(plan(l, p) == SVO_OK && l.C == C, "%s", what);
      const int G = C <= 128 ? 1 : (C + 127) / 128;
      CHECK(l.G == G && l.CPW == (C > 2048 ? G : 1) && l.GS == (C > 2048 ? 1 : G) && l.NG == (C > 2048 ? (C + G - 1) / G : C), "%s: G %d CPW %d GS %d NG %d", what, l.G, l.CPW, l.GS, l.NG);
    }
    CHECK(l.G == 17 && l.NG == 121, "2,049 chunks: G %d, NG %d", l.G, l.NG);
    // K = 12: 2,741 wire elements, 2,744 granules = 43,904 bytes per partial; one per chunk while the store stays within 64 MB:
    // 1,528 chunks are 67,085,312 bytes, 1,529 are 67,129,216 (64 MB = 67,108,864)
    Problem w;
    w.K = 12;
    for (int j = 0; j < 64 * 1528; ++j) w.landmark({1 + j % 11});
    CHECK(plan(l, w) == SVO_OK && l.E == 2741 && l.Epad == 2744 && l.C == 1528 && l.G == 12 && l.CPW == 1 && l.GS == 12 && l.NG == 1528, "K = 12, 1,528 chunks: E %d G %d CPW %d", l.E, l.G, l.CPW);
    for (int j = 0; j < 64; ++j) w.landmark({1});
    CHECK(plan(l, w) == SVO_OK && l.C == 1529 && l.G == 12 && l.CPW == 12 && l.GS == 1 && l.NG == 128, "K = 12, 1,529 chunks: G %d CPW %d NG %d", l.G, l.CPW, l.NG);
  }
  // ---- rejections, each at its boundary, leave no problem behind
  {
    BaLayout l;
    Problem ok;
    ok.K = 3;
    ok.landmark({0, 2});
    ok.landmark({1});
    ok.landmark({0, 1, 2});
    CHECK(plan(l, ok) == SVO_OK && l.K == 3, "the problem the rejections start from");
    Problem p = ok;
    std::swap(p.oj[2], p.oj[3]);  // landmarks 0 0 2 1 2 2
    rejected(l, p, "ba: observations must be sorted by landmark", "unsorted");
    p = ok; p.oj[2] = 0;          // 0 0 0 2 2 2: equal neighbours are sorted
    CHECK(plan(l, p) == SVO_OK, "equal landmark indices are sorted");
    p = ok; p.op[1] = 3;
    rejected(l, p, "ba: observation index out of range", "pose K");
    p = ok; p.op[1] = -1;
    rejected(l, p, "ba: observation index out of range", "pose -1");
    p = ok; p.oj[5] = 3;
    rejected(l, p, "ba: observation index out of range", "landmark npts");
    p = ok; p.oj[0] = -1;
    rejected(l, p, "ba: observation index out of range", "landmark -1");
    p = ok; p.op[1] = 2; p.oj[5] = 2;
    CHECK(plan(l, p) == SVO_OK, "pose K - 1 and landmark npts - 1 are in range");
    Problem many;
    many.K = 2;
    many.landmark({1});
    many.landmark(std::vector<int>(64, 1));
    CHECK(plan(l, many) == SVO_OK && l.C == 2, "64 observations of one landmark");
    check_plan(many, l, "64 observations of one landmark");
    many.landmark(std::vector<int>(65, 1));
    rejected(l, many, "ba: a landmark has more than 64 observations", "65 observations of one landmark");
  }
  if (fails) { fprintf(stderr, "%d check(s) failed\n", fails); return 1; }
  printf("ba layout ok\n");
  return 0;
}
