// The class rule of -trio (csrc/mfx_trio.h: the role tag, the head walk over the tagged merged run, mfx_trio_rule, the histogram columns,
// the whole of mfx_trio_host) under AddressSanitizer + UBSan, against a plain walk over the union of the three key sets that restates the
// specification (include/merfin_amd.h, at mfx_db_trio): empty inputs, single k-mers, every one of the seven membership patterns, a k-mer at
// the very end of every run, the largest 31-mers (the tagged key uses all 64 bits), counts of 1, at the cutoffs, 2^32 - 1, cutoffs of 1 and
// of 2^32 - 1, max_mult 4 and 65536, with and without a child, and random worlds.  No device, no library.
//   g++ -fsanitize=address,undefined -static-libasan -static-libubsan -g -O1 -std=c++17 -Wall -Werror -Imerfin_amd/csrc -Iinclude
//       tools/native/trio_sanitize.cpp -o /tmp/trio_sanitize && /tmp/trio_sanitize
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <vector>
#include "mfx_trio.h"

static int bad = 0, cases = 0;

struct Db { std::vector<uint64_t> k; std::vector<uint32_t> v; };

static Db make(const std::map<uint64_t, uint32_t> &m) {
  Db d;
  for (const auto &e : m) { d.k.push_back(e.first); d.v.push_back(e.second); }
  return d;
}

// the specification, k-mer by k-mer
static void plain(const Db db[3], const mfx_trio_cuts &t, uint32_t max_mult, mfx_trio_host_result &R) {
  std::map<uint64_t, uint32_t> c[3];
  std::map<uint64_t, int> all;
  for (int r = 0; r < 3; ++r)
    for (size_t i = 0; i < db[r].k.size(); ++i) { c[r][db[r].k[i]] = db[r].v[i]; all[db[r].k[i]] = 1; }
  const uint64_t W = (uint64_t)max_mult + 1;
  R.img.assign(3 * W, 0);
  auto col = [&](uint32_t x) { return x < max_mult ? x : max_mult; };
  for (const auto &e : all) {
    const uint64_t key = e.first;
    const uint32_t cm = c[0].count(key) ? c[0][key] : 0u, cp = c[1].count(key) ? c[1][key] : 0u, cc = c[2].count(key) ? c[2][key] : 0u;
    if (cm && !cp) { ++R.img[0 * W + col(cm)]; ++R.stats[MFX_TRIO_S_MAT_ONLY]; if (cm >= t.tm) ++R.stats[MFX_TRIO_S_MAT_CUT]; }
    if (cp && !cm) { ++R.img[1 * W + col(cp)]; ++R.stats[MFX_TRIO_S_PAT_ONLY]; if (cp >= t.tp) ++R.stats[MFX_TRIO_S_PAT_CUT]; }
    if (cm && cp) ++R.stats[MFX_TRIO_S_BOTH];
    if (cc) ++R.img[2 * W + col(cc)];
    const bool child_ok = !t.has_child || (cc && cc >= t.tc);
    if (t.has_child && cc && cc >= t.tc) ++R.stats[MFX_TRIO_S_CHILD_CUT];
    if (cm >= t.tm && cm && !cp && child_ok) { R.ak.push_back(key); R.av.push_back(t.has_child && cc < cm ? cc : cm); }
    if (cp >= t.tp && cp && !cm && child_ok) { R.bk.push_back(key); R.bv.push_back(t.has_child && cc < cp ? cc : cp); }
  }
}

static void check(const char *name, const Db &mat, const Db &pat, const Db &child, bool has_child, uint32_t tm, uint32_t tp, uint32_t tc, uint32_t max_mult) {
  ++cases;
  const Db db[3] = {mat, pat, has_child ? child : Db{}};
  const mfx_trio_cuts t{tm, tp, tc, has_child};
  // (exact-size copies on the heap: a read one past a run's end is an error under AddressSanitizer)
  std::vector<uint64_t> k0(db[0].k), k1(db[1].k), k2(db[2].k);
  std::vector<uint32_t> v0(db[0].v), v1(db[1].v), v2(db[2].v);
  k0.shrink_to_fit(); k1.shrink_to_fit(); k2.shrink_to_fit(); v0.shrink_to_fit(); v1.shrink_to_fit(); v2.shrink_to_fit();
  const uint64_t *const keys[3] = {k0.data(), k1.data(), k2.data()};
  const uint32_t *const vals[3] = {v0.data(), v1.data(), v2.data()};
  const uint64_t n[3] = {k0.size(), k1.size(), k2.size()};
  mfx_trio_host_result got, want;
  mfx_trio_host(keys, vals, n, t, max_mult, got);
  plain(db, t, max_mult, want);
  bool ok = got.ak == want.ak && got.av == want.av && got.bk == want.bk && got.bv == want.bv && got.img == want.img;
  for (int s = 0; s < MFX_TRIO_NSTATS; ++s) ok = ok && got.stats[s] == want.stats[s];
  if (!ok) {
    ++bad;
    printf("MISMATCH %s (child %d, cuts %u %u %u, max_mult %u): A %zu / %zu, B %zu / %zu\n", name, (int)has_child, tm, tp, tc, max_mult, got.ak.size(), want.ak.size(),
           got.bk.size(), want.bk.size());
  }
}

static void every_way(const char *name, const Db &mat, const Db &pat, const Db &child) {
  static const uint32_t cuts[][3] = {{1, 1, 1}, {2, 3, 2}, {5, 5, 5}, {0xffffffffu, 0xffffffffu, 0xffffffffu}, {1, 0xffffffffu, 3}};
  for (const auto &c : cuts)
    for (uint32_t max_mult : {4u, 16u, 65536u}) {
      check(name, mat, pat, child, true, c[0], c[1], c[2], max_mult);
      check(name, mat, pat, child, false, c[0], c[1], 1, max_mult);
    }
}

int main() {
  const uint32_t TOP = 0xffffffffu;
  const uint64_t END31 = (1ull << 62) - 1;                      // the largest 31-mer
  every_way("nothing", Db{}, Db{}, Db{});
  every_way("one in mat", make({{7, 3}}), Db{}, Db{});
  every_way("one in pat", Db{}, make({{7, 3}}), Db{});
  every_way("one in child", Db{}, Db{}, make({{7, 3}}));
  every_way("one in all", make({{7, 3}}), make({{7, 4}}), make({{7, 2}}));
  // the seven membership patterns, counts around the cutoffs, the last k-mer of every run shared in a different way
  every_way("patterns", make({{1, 1}, {2, 2}, {3, 5}, {5, 2}, {7, TOP}, {9, 4}, {END31 - 2, 6}, {END31, 2}}),
            make({{1, 3}, {4, 3}, {5, 2}, {6, TOP}, {9, 1}, {END31 - 1, 5}, {END31, 9}}),
            make({{2, 1}, {3, 7}, {4, 2}, {6, 5}, {8, 1}, {9, 9}, {END31 - 2, TOP}, {END31 - 1, 5}, {END31, 1}}));
  every_way("top of the key space", make({{END31 - 1, 2}, {END31, 3}}), make({{END31 - 1, 2}}), make({{END31, TOP}}));
  every_way("zero and the top", make({{0, 2}, {END31, 3}}), make({{0, 1}}), make({{0, 5}, {END31, 1}}));
  std::mt19937_64 rng(12345);
  for (int w = 0; w < 40; ++w) {
    const uint64_t space = w % 3 == 0 ? 50 : w % 3 == 1 ? 5000 : END31;
    const size_t sizes[3] = {(size_t)(rng() % 600), (size_t)(rng() % 600), (size_t)(rng() % 600)};
    std::map<uint64_t, uint32_t> m[3];
    std::vector<uint64_t> pool;
    for (int i = 0; i < 900; ++i) pool.push_back(space == END31 ? (rng() & END31) : rng() % space);
    for (int r = 0; r < 3; ++r)
      for (size_t i = 0; i < sizes[r]; ++i) m[r][pool[rng() % pool.size()]] = rng() % 20 == 0 ? TOP - (uint32_t)(rng() % 2) : 1u + (uint32_t)(rng() % 30);
    every_way("random", make(m[0]), make(m[1]), make(m[2]));
  }
  printf("%s (%d mismatches, %d cases)\n", bad ? "FAILED" : "OK", bad, cases);
  return bad ? 1 : 0;
}
