// The layout of a landmark-major bundle-adjustment problem on the device, free of the GPU — the host half of the declared
// summation order (oracle/ora_ba.cpp, "chunk order"): landmark CSR, wave chunks of <= 64 observations made of whole landmarks,
// the dimensions of the partial store, per chunk the destination tables the owner lanes walk, and the one staging image
// [points | points (candidate copy) | per-slot records | per-slot uv | chunk tables | table offsets | keys | poses x 2] that goes
// to the device in one copy.  csrc/ba.hip plans, sizes its arena, fills the image and hands `device base + offset` pointers to
// the kernels; tests/sanitize/ba_layout_test.cpp walks plan() and write_image() on a CPU.
#ifndef SVO_BA_LAYOUT_H_
#define SVO_BA_LAYOUT_H_
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "svo.h"

// One observation slot (slot = 64 * chunk + lane; chunks are padded to a full wave): the kernels read it as an int4.
struct BaSlotRec { int32_t pose /* -1: padding lane */, landmark, first /* lane of the landmark's segment */, len; };

struct BaLayout {
  int K = 0, n = 0, M = 0, L = 0, C = 0;   // poses, 6 (K - 1), observations, landmarks, chunks; K = 0: no problem planned
  int G = 1, NG = 0, Epad = 0, E = 0;      // chunks per declared group, partials in the store, granules per partial (E rounded up), wire-format elements
  int CPW = 1, GS = 1;                     // chunks per stored partial (1, or G for very large problems), stored partials per declared group (G / CPW)
  int det = 0;                             // deterministic mode: chunk tables + partial store
  bool mfma_ok = false;                    // bulk problem eligible for the MFMA linearisation (n <= 128, one observation per (landmark, pose))
  int tab_max_words = 0;                   // largest chunk table (u16 words)
  double flops_iter = 0, bytes_iter = 0;   // SURVEY 8(d) algorithmic f64 flops / bytes of ONE LM iteration
  std::vector<int32_t> lm_start, chunks;   // landmark CSR (L + 1), first observation of every chunk (C + 1)
  std::vector<uint16_t> tab;               // chunk tables back to back (u16 words)
  std::vector<uint32_t> tab_off;           // C + 1 offsets into tab
  bool with_keys = false;
  size_t o_pts = 0, o_cpts = 0, o_rec = 0, o_uv = 0, o_tab = 0, o_toff = 0, o_key = 0, o_p0 = 0, o_p1 = 0, total = 0;  // image offsets, 256-byte aligned

  // Destination index of pose-pair block (ka <= kb) among the F (F + 1) / 2 upper blocks, row-major.
  static int upper_index(int ka, int kb, int F) { return ka * F - ka * (ka - 1) / 2 + (kb - ka); }
  size_t image_bytes() const { return (total + 15) & ~(size_t)15; }
  // host-driven kernels: u16 words of LDS for the workgroup's chunk table (8 KB at most; 0: read from global memory)
  int tab_lds_words() const { return (det && tab_max_words > 0 && tab_max_words <= 4096) ? ((tab_max_words + 3) & ~3) : 0; }
  void clear() { K = n = M = L = C = 0; }

  // Observations (op: pose, oj: landmark) sorted by landmark; `accumulation`: SVO_BA_ACC_*; with_keys: the image carries a key
  // per landmark.  Returns SVO_OK, or SVO_ERR_INVALID with *err set and no problem planned.  Scratch vectors are members: a
  // keyframe's solve allocates nothing.
  int plan(int K_, int npts, int M_, const int32_t* op, const int32_t* oj, int accumulation, bool with_keys_, const char** err) {
    clear();
#define BA_LAYOUT_REQUIRE(cond, msg) do { if (!(cond)) { *err = (msg); clear(); return SVO_ERR_INVALID; } } while (0)
    lm_start.assign((size_t)npts + 1, 0);
    chunks.clear();
    for (int o = 0; o < M_; ++o) {
      BA_LAYOUT_REQUIRE(oj[o] >= 0 && oj[o] < npts && op[o] >= 0 && op[o] < K_, "ba: observation index out of range");
      BA_LAYOUT_REQUIRE(o == 0 || oj[o] >= oj[o - 1], "ba: observations must be sorted by landmark");
      lm_start[oj[o] + 1]++;
    }
    for (int j = 0; j < npts; ++j) {
      BA_LAYOUT_REQUIRE(lm_start[j + 1] <= 64, "ba: a landmark has more than 64 observations");
      lm_start[j + 1] += lm_start[j];
    }
    K = K_; n = 6 * (K_ - 1); M = M_; L = npts;
    // chunks (declared with the summation order, oracle/ora_ba.cpp): whole landmarks, greedily, at most 64 observations each
    chunks.push_back(0);
    int cur = 0;
    for (int j = 0; j < npts; ++j) {
      const int len = lm_start[j + 1] - lm_start[j];
      if (len == 0) continue;
      if (cur + len > 64) { chunks.push_back(lm_start[j]); cur = 0; }
      cur += len;
    }
    chunks.push_back(M);
    C = (int)chunks.size() - 1;
    {
      // 466 flops per observation + per landmark 50 + 144 L + 216 L (L + 1) / 2; 24 B per observation, 48 B per landmark, 56 B per pose
      double fl = 466.0 * M;
      int n_seen = 0;
      for (int j = 0; j < npts; ++j) {
        const double Lj = lm_start[j + 1] - lm_start[j];
        if (Lj > 0) { fl += 50.0 + 144.0 * Lj + 108.0 * Lj * (Lj + 1.0); ++n_seen; }
      }
      flops_iter = fl;
      bytes_iter = 24.0 * M + 48.0 * n_seen + 56.0 * K;
    }
    tab.clear(); tab_off.clear();
    tab_max_words = 0;
    const int F = K - 1;
    bool dup = false;
    for (int j = 0; j < npts; ++j) {
      uint64_t seen = 0;
      for (int o = lm_start[j]; o < lm_start[j + 1]; ++o) {
        const uint64_t bit = 1ull << op[o];
        dup |= (seen & bit) != 0;
        seen |= bit;
      }
    }
    // deterministic mode ("chunk order"): G chunks per group, NG groups, E wire elements; the partial store holds E x NG granules
    const int nU = F * (F + 1) / 2;
    G = C <= 128 ? 1 : (C + 127) / 128;
    // partials in the store: one per chunk (the groups of G are applied by the level-2 sums) while that stays below 64 MB —
    // a 1280x720 window: 1,500 chunks x 1,920 elements = 46 MB; config 4 (6,900 chunks x 7,472 elements) keeps one partial per GROUP
    // (and at most 2,048 partials: the level-2 reducers hold all partials of an element in 4,096 doubles of LDS)
    CPW = ((size_t)((36 * nU + 33 * F + 2 + 7) & ~7) * (size_t)C * 16 <= ((size_t)64 << 20) && C <= 2048) ? 1 : G;
    GS = G / CPW;
    NG = C > 0 ? (C + CPW - 1) / CPW : 0;
    E = 36 * nU + 33 * F + 2;
    Epad = (E + 7) & ~7;
    det = (size_t)Epad * (size_t)(NG > 0 ? NG : 1) * 16 <= ((size_t)512 << 20) ? 1 : 0;
    if (accumulation == SVO_BA_ACC_ATOMICS || accumulation == SVO_BA_ACC_MFMA) det = 0;
    BA_LAYOUT_REQUIRE(!(accumulation == SVO_BA_ACC_DETERMINISTIC && !det), "ba: problem too large for deterministic accumulation");
    mfma_ok = !dup && n <= 128 && n > 0 && accumulation != SVO_BA_ACC_ATOMICS;
    BA_LAYOUT_REQUIRE(!(accumulation == SVO_BA_ACC_MFMA && !mfma_ok), "ba: MFMA accumulation needs <= 22 poses and one observation per (landmark, pose)");
#undef BA_LAYOUT_REQUIRE
    if (det) build_tables(op, oj, F, nU);
    // ---- the staging image
    const size_t nslots = (size_t)C * 64;
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    size_t off = 0;
    o_pts = off; off = al(off + sizeof(double) * 3 * (size_t)npts);
    o_cpts = off; off = al(off + sizeof(double) * 3 * (size_t)npts);
    o_rec = off; off = al(off + sizeof(BaSlotRec) * nslots);
    o_uv = off; off = al(off + sizeof(double) * 2 * nslots);
    o_tab = off; off = al(off + sizeof(uint16_t) * tab.size());
    o_toff = off; off = al(off + sizeof(uint32_t) * tab_off.size());
    with_keys = with_keys_;
    o_key = off; if (with_keys) off = al(off + sizeof(unsigned) * (size_t)npts);
    o_p0 = off; off = al(off + sizeof(double) * 7 * (size_t)K);
    o_p1 = off; off = al(off + sizeof(double) * 7 * (size_t)K);
    total = off;
    return SVO_OK;
  }

  // Fills image_bytes() at `h` for the planned problem: op, oj as plan() saw them; lm_ids (the keys' source) only with_keys.
  void write_image(uint8_t* h, const int32_t* op, const int32_t* oj, const double* points3, const double* poses7, const double* uv,
                   const int64_t* lm_ids) const {
    if (L) { memcpy(h + o_pts, points3, sizeof(double) * 3 * (size_t)L); memcpy(h + o_cpts, points3, sizeof(double) * 3 * (size_t)L); }
    BaSlotRec* rec = reinterpret_cast<BaSlotRec*>(h + o_rec);
    double* suv = reinterpret_cast<double*>(h + o_uv);
    for (int c = 0; c < C; ++c) {
      const int c0 = chunks[c], c1 = chunks[c + 1];
      for (int lane = 0; lane < 64; ++lane) {
        const size_t slot = (size_t)c * 64 + lane;
        const int o = c0 + lane;
        if (o < c1) {
          const int j = oj[o];
          rec[slot] = BaSlotRec{op[o], j, lm_start[j] - c0, lm_start[j + 1] - lm_start[j]};
          suv[2 * slot] = uv[2 * (size_t)o]; suv[2 * slot + 1] = uv[2 * (size_t)o + 1];
        } else {
          rec[slot] = BaSlotRec{-1, 0, lane, 0};
          suv[2 * slot] = 0.0; suv[2 * slot + 1] = 0.0;
        }
      }
    }
    if (!tab.empty()) memcpy(h + o_tab, tab.data(), sizeof(uint16_t) * tab.size());
    if (!tab_off.empty()) memcpy(h + o_toff, tab_off.data(), sizeof(uint32_t) * tab_off.size());
    if (with_keys) { unsigned* k = reinterpret_cast<unsigned*>(h + o_key); for (int j = 0; j < L; ++j) k[j] = (unsigned)lm_ids[(size_t)j]; }
    memcpy(h + o_p0, poses7, sizeof(double) * 7 * (size_t)K);
    memcpy(h + o_p1, poses7, sizeof(double) * 7 * (size_t)K);
  }

 private:
  std::vector<int32_t> cnt_;  // fill cursors: nU block lists, then F pose lists

  // Chunk tables (ChunkTab): per chunk the pair entries of every UPPER pose-pair block in (landmark, i, t) order — pair
  // (i, t >= i) enters block (k_i, k_t) when k_i <= k_t and, transposed, block (k_t, k_i) when t != i and k_t <= k_i (two
  // observations of one landmark in one pose: both, the direct entry first) — and the lanes of every free pose.
  // Per table: nU + 1 entry offsets | F + 1 lane offsets | entries (lane i | transposed 0x80 | lane t << 8) | lanes (u8).
  void build_tables(const int32_t* op, const int32_t* oj, int F, int nU) {
    std::vector<int32_t>& cur = cnt_;
    tab_off.reserve((size_t)C + 1);
    tab.reserve((size_t)M * 3 + (size_t)C * (size_t)(nU + F + 4));
    for (int c = 0; c < C; ++c) {
      const int c0 = chunks[c], c1 = chunks[c + 1];
      cur.assign((size_t)nU + (size_t)F + 2, 0);
      // pass 1: list lengths
      for (int i = c0; i < c1; ++i) {
        const int ki = op[i] - 1;
        if (ki < 0) continue;
        cur[nU + ki]++;
        const int o1 = lm_start[oj[i] + 1];
        for (int t = i; t < o1; ++t) {
          const int kt = op[t] - 1;
          if (kt < 0) continue;
          if (ki <= kt) cur[upper_index(ki, kt, F)]++;
          if (t != i && kt <= ki) cur[upper_index(kt, ki, F)]++;
        }
      }
      tab_off.push_back((uint32_t)tab.size());
      const size_t t0 = tab.size();
      int n_ent = 0, n_free = 0;
      for (int q = 0; q < nU; ++q) { const int len = cur[q]; cur[q] = n_ent; tab.push_back((uint16_t)n_ent); n_ent += len; }
      tab.push_back((uint16_t)n_ent);
      for (int k = 0; k < F; ++k) { const int len = cur[nU + k]; cur[nU + k] = n_free; tab.push_back((uint16_t)n_free); n_free += len; }
      tab.push_back((uint16_t)n_free);
      const size_t e_at = tab.size();
      tab.resize(e_at + (size_t)n_ent + (size_t)((n_free + 1) / 2), 0);
      uint16_t* ent = tab.data() + e_at;
      uint8_t* plane = reinterpret_cast<uint8_t*>(ent + n_ent);
      // pass 2: fill, every list in (landmark, i, t) / lane order
      for (int i = c0; i < c1; ++i) {
        const int ki = op[i] - 1;
        if (ki < 0) continue;
        plane[cur[nU + ki]++] = (uint8_t)(i - c0);
        const int o1 = lm_start[oj[i] + 1];
        for (int t = i; t < o1; ++t) {
          const int kt = op[t] - 1;
          if (kt < 0) continue;
          if (ki <= kt) ent[cur[upper_index(ki, kt, F)]++] = (uint16_t)((i - c0) | ((t - c0) << 8));
          if (t != i && kt <= ki) ent[cur[upper_index(kt, ki, F)]++] = (uint16_t)((i - c0) | 0x80 | ((t - c0) << 8));
        }
      }
      if ((tab.size() - t0) & 1) tab.push_back(0);  // tables start on even u16 offsets (read as 32-bit words)
      tab_max_words = std::max(tab_max_words, (int)(tab.size() - t0));
    }
    tab_off.push_back((uint32_t)tab.size());
  }
};

#endif
