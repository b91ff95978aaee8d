// The host text of -diploid (csrc/mfx_diploid.h: the role tag, the merge of the two assemblies, the head compaction into the pair run, the
// tiled lane walk of csrc/mfx_join.h with a 64-bit asm value, mfx_dip_rule, the counters, the piece sums) under AddressSanitizer + UBSan,
// against a plain walk over the union of the three key sets that restates the specification (include/merfin_amd.h, at mfx_db_diploid): empty
// inputs, single k-mers, the seven membership patterns, counts of 2^32 - 1 in both assemblies (cb clamps), the largest 31-mers (the tagged
// key uses all 64 bits), -min / -max, a k-mer of all three inputs on every lane and tile boundary of the join's merged order and of the pair
// step's merged order, and random worlds of several tiles.  No device, no library.
//   g++ -fsanitize=address,undefined -static-libasan -static-libubsan -g -O1 -std=c++17 -Wall -Werror -Imerfin_amd/csrc -Iinclude
//       tools/native/diploid_sanitize.cpp -o /tmp/diploid_sanitize && /tmp/diploid_sanitize
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <vector>
#include "mfx_diploid.h"
#include "mfx_kstar.h"

static int bad = 0, cases = 0;

struct Db { std::vector<uint64_t> k; std::vector<uint32_t> v; };

static Db make(const std::map<uint64_t, uint32_t> &m) {
  Db d;
  for (const auto &e : m) { d.k.push_back(e.first); d.v.push_back(e.second); }
  return d;
}

struct Plain {
  std::vector<uint64_t> asm_img, cn_img, keys;
  uint64_t n_entries = 0, stats[MFX_DIP_NSTATS] = {};
  double tot[64] = {}, und[3][64] = {};
};

static double readK(double peak, uint32_t r) { double rk, pr; mfx_getK_core(peak, 0, nullptr, nullptr, r, rk, pr); return rk; }

// the specification, k-mer by k-mer
static void plain(const Db db[3], int k, uint64_t lo, uint64_t hi, uint32_t copies, uint32_t max_mult, double peak, Plain &R) {
  std::map<uint64_t, uint32_t> c[3];
  std::map<uint64_t, int> all;
  for (int r = 0; r < 3; ++r)
    for (size_t i = 0; i < db[r].k.size(); ++i) { c[r][db[r].k[i]] = db[r].v[i]; all[db[r].k[i]] = 1; }
  const uint64_t W = (uint64_t)max_mult + 1;
  R.asm_img.assign(4 * W, 0);
  R.cn_img.assign((copies + 2) * W, 0);
  const int shift = 2 * k >= 6 ? 2 * k - 6 : 0;
  for (const auto &e : all) {
    const uint64_t key = e.first;
    const uint64_t r = c[0].count(key) ? c[0][key] : 0u, c1 = c[1].count(key) ? c[1][key] : 0u, c2 = c[2].count(key) ? c[2][key] : 0u;
    const uint64_t rf = (r < lo || r > hi) ? 0 : r, cb = c1 + c2 > 0xffffffffull ? 0xffffffffull : c1 + c2;
    const uint64_t cx[3] = {c1, c2, cb};
    R.keys.push_back(key);
    if (rf || cb) {
      const uint64_t col = rf < max_mult ? rf : max_mult;
      ++R.asm_img[(c1 ? (c2 ? 3 : 1) : (c2 ? 2 : 0)) * W + col];
      ++R.cn_img[(cb <= copies ? cb : copies + 1) * W + col];
      ++R.n_entries;
    }
    for (int x = 0; x < 3; ++x) {
      if (!cx[x]) continue;
      uint64_t *s = R.stats + x * MFX_DIP_PER_X;
      ++s[MFX_DIP_DISTINCT];
      s[MFX_DIP_TOTAL] += cx[x];
      if (!r) { ++s[MFX_DIP_ONLY_DISTINCT]; s[MFX_DIP_ONLY_TOTAL] += cx[x]; }
      if (rf) ++s[MFX_DIP_FOUND];
    }
    if (rf) ++R.stats[MFX_DIP_SOLID];
    if (r) ++R.stats[MFX_DIP_N_READ];
    if (c1 && c2) ++R.stats[MFX_DIP_N_SHARED];
    if (r) {
      const double K = readK(peak, (uint32_t)r);
      const int piece = (int)((key >> shift) & 63u);
      R.tot[piece] += K;
      for (int x = 0; x < 3; ++x)
        if (K > (double)cx[x]) R.und[x][piece] += K - (double)cx[x];
    }
  }
}

static void check(const char *name, const Db &reads, const Db &h1, const Db &h2, int k, uint64_t lo, uint64_t hi, uint32_t copies, uint32_t max_mult) {
  ++cases;
  const Db db[3] = {reads, h1, h2};
  const double peak = 3.3;
  // (exact-size copies on the heap: a read one past a run's end is an error under AddressSanitizer)
  std::vector<uint64_t> k0(db[0].k), k1(db[1].k), k2(db[2].k);
  std::vector<uint32_t> v0(db[0].v), v1(db[1].v), v2(db[2].v);
  k0.shrink_to_fit(); k1.shrink_to_fit(); k2.shrink_to_fit(); v0.shrink_to_fit(); v1.shrink_to_fit(); v2.shrink_to_fit();
  mfx_dip_host_result got;
  std::vector<uint64_t> keys;
  bool ok = true;
  mfx_dip_host(k0.data(), v0.data(), k0.size(), k1.data(), v1.data(), k1.size(), k2.data(), v2.data(), k2.size(), k, lo, hi, copies, max_mult, true,
               [&](uint32_t r) { return readK(peak, r); }, [&](uint64_t key, uint32_t, uint32_t, uint32_t) { keys.push_back(key); }, got);
  Plain want;
  plain(db, k, lo, hi, copies, max_mult, peak, want);
  ok = ok && keys == want.keys && got.asm_img == want.asm_img && got.cn_img == want.cn_img && got.n_entries == want.n_entries;
  for (uint32_t s = 0; s < MFX_DIP_NSTATS; ++s) ok = ok && got.stats[s] == want.stats[s];
  for (int p = 0; p < 64; ++p) {
    ok = ok && got.tot[p] == want.tot[p];
    for (int x = 0; x < 3; ++x) ok = ok && got.und[x][p] == want.und[x][p];
  }
  if (!ok) {
    ++bad;
    printf("MISMATCH %s (k %d, -min %llu -max %llu, copies %u, max_mult %u): %zu / %zu k-mers, %llu / %llu entries\n", name, k, (unsigned long long)lo,
           (unsigned long long)hi, copies, max_mult, keys.size(), want.keys.size(), (unsigned long long)got.n_entries, (unsigned long long)want.n_entries);
  }
}

static void every_way(const char *name, const Db &reads, const Db &h1, const Db &h2, int k) {
  check(name, reads, h1, h2, k, 0, 0xffffffffull, 4, 10000);
  check(name, reads, h1, h2, k, 2, 50, 1, 4);
  check(name, reads, h1, h2, k, 0, 0xffffffffull, 6, 16);
  check(name, h1, reads, h2, k, 1, 7, 2, 65536);              // (the roles turned)
}

// tests/test_join_cpu.py::boundary_world with a third input: in the merged order of runs A and B a k-mer of both stands at position p (A's
// record; B's twin at p + 1) wherever (p + shift) % grain == grain - 1; the k-mer is then also given to C.  join: A the reads, B the pair run
// (its k-mers dealt to hap1, hap2 or both), C both assemblies.  Else: A hap1, B hap2, C the reads.
static void boundary(uint32_t grain, uint32_t shift, uint32_t total, bool join, Db db[3]) {
  std::mt19937_64 rng(grain * 31 + shift);
  std::map<uint64_t, uint32_t> m[3];
  uint64_t key = 10;
  uint32_t p = 0, n = 0;
  while (p < total) {
    const uint32_t cnt = 1 + (n++ % 7);
    if ((p + shift) % grain == grain - 1) {
      m[0][key] = 100 + cnt; m[1][key] = cnt; m[2][key] = cnt + 1;
      p += 2;
    } else {
      const bool a = (p / 3) % 2;
      if (join) {
        if (a) m[0][key] = 100 + cnt;
        else { if (n % 3 != 1) m[1][key] = cnt; if (n % 3 != 0) m[2][key] = cnt + 2; }
      } else {
        m[a ? 1 : 2][key] = cnt;
        if (n % 5 == 0) m[0][key] = 100 + cnt;
      }
      p += 1;
    }
    key += 1 + rng() % 3;
  }
  for (int r = 0; r < 3; ++r) db[r] = make(m[r]);
}

int main() {
  const uint32_t TOP = 0xffffffffu;
  const uint64_t END31 = (1ull << 62) - 1;                      // the largest 31-mer
  every_way("nothing", Db{}, Db{}, Db{}, 21);
  every_way("one in the reads", make({{7, 3}}), Db{}, Db{}, 21);
  every_way("one in hap1", Db{}, make({{7, 3}}), Db{}, 21);
  every_way("one in hap2", Db{}, Db{}, make({{7, 3}}), 21);
  every_way("one in all", make({{7, 3}}), make({{7, 4}}), make({{7, 2}}), 21);
  every_way("patterns", make({{1, 1}, {2, 2}, {3, 5}, {5, 2}, {7, TOP}, {9, 4}, {END31 - 2, 6}, {END31, 2}}),
            make({{1, 3}, {4, 3}, {5, 2}, {6, TOP}, {9, 1}, {END31 - 1, 5}, {END31, 9}}),
            make({{2, 1}, {3, 7}, {4, 2}, {6, 5}, {8, 1}, {9, 9}, {END31 - 2, TOP}, {END31 - 1, 5}, {END31, 1}}), 31);
  every_way("cb clamps", make({{5, 60}, {END31, TOP}}), make({{5, TOP}, {6, TOP}, {END31, TOP}}), make({{5, TOP}, {6, TOP - 1}, {END31, 1}}), 31);
  every_way("zero and the top", make({{0, 2}, {END31, 3}}), make({{0, 1}}), make({{0, 5}, {END31, 1}}), 31);
  every_way("k = 2", make({{0, 20}, {3, 1}, {15, 40}}), make({{3, 1}, {4, 2}, {15, 1}}), make({{0, 1}, {15, 2}}), 2);
  for (uint32_t grain : {MFX_JOIN_PER, MFX_JOIN_TILE})
    for (uint32_t shift : {0u, 1u, grain - 1u})
      for (bool join : {true, false}) {
        Db db[3];
        boundary(grain, shift, 2 * MFX_JOIN_TILE + 5 * MFX_JOIN_PER + 3, join, db);
        check(join ? "boundary of the join" : "boundary of the pair step", db[0], db[1], db[2], 21, 0, TOP, 4, 1000);
      }
  std::mt19937_64 rng(4711);
  for (int w = 0; w < 24; ++w) {
    const uint64_t space = w % 3 == 0 ? 3000 : w % 3 == 1 ? 40000 : END31;
    const size_t top = w % 4 == 0 ? 6000 : 700;
    const size_t sizes[3] = {(size_t)(rng() % top), (size_t)(rng() % top), (size_t)(rng() % top)};
    std::map<uint64_t, uint32_t> m[3];
    std::vector<uint64_t> pool;
    for (size_t i = 0; i < top + top / 2; ++i) pool.push_back(space == END31 ? (rng() & END31) : rng() % space);
    for (int r = 0; r < 3; ++r)
      for (size_t i = 0; i < sizes[r]; ++i) m[r][pool[rng() % pool.size()]] = rng() % 20 == 0 ? TOP - (uint32_t)(rng() % 2) : 1u + (uint32_t)(rng() % 30);
    every_way("random", make(m[0]), make(m[1]), make(m[2]), space == END31 ? 31 : 21);
  }
  printf("%s (%d mismatches, %d cases)\n", bad ? "FAILED" : "OK", bad, cases);
  return bad ? 1 : 0;
}
