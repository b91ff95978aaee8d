// cuts_sanitize.cpp -- mfx_cut_bins of csrc/mfx_grow.h under AddressSanitizer + UBSan (tests/test_cuts_cpu.py builds and runs it): the
// key ranges of the passes of a count, each cutting checked for "ascending, complete, no range without entries, largest part minimal", and
// on small inputs against every cutting there is.  Prints one line per case and exits non-zero on a mismatch.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../merfin_amd/csrc/mfx_grow.h"

typedef unsigned __int128 u128;

static int g_bad = 0, g_cases = 0;
static void check(bool ok, const char *what, unsigned long long a, unsigned long long b, unsigned long long c) {
  ++g_cases;
  printf("%s %s (%llu, %llu, %llu)\n", ok ? "ok      " : "MISMATCH", what, a, b, c);
  if (!ok) ++g_bad;
}

static u128 mass(const std::vector<uint64_t> &bins, uint32_t lo, uint32_t hi) {
  u128 s = 0;
  for (uint32_t b = lo; b < hi; ++b) s += bins[b];
  return s;
}

// the fewest consecutive ranges of mass <= T that hold [lo, hi): each taken as long as T allows (0xffffffff: a bin alone exceeds T)
static uint32_t fewest_slow(const std::vector<uint64_t> &bins, uint32_t lo, uint32_t hi, u128 T) {
  uint32_t n = 0;
  for (uint32_t b = lo; b < hi;) {
    if (bins[b] > T) return 0xffffffffu;
    u128 s = 0;
    while (b < hi && s + bins[b] <= T) s += bins[b++];
    ++n;
  }
  return n;
}

// ascending, complete, no range without entries, as many ranges as the rule gives, n the range's mass, the largest part minimal
static bool cutting_ok(const std::vector<uint64_t> &bins, uint32_t lo, uint32_t hi, uint32_t parts, const std::vector<mfx_bin_range> &out) {
  uint32_t nonempty = 0;
  for (uint32_t b = lo; b < hi; ++b) nonempty += bins[b] != 0;
  const uint32_t want = parts < nonempty ? parts : nonempty;
  if (out.size() != want) return false;
  if (want == 0) return true;
  if (out.front().bin_lo != lo || out.back().bin_hi != hi) return false;
  u128 largest = 0;
  for (size_t i = 0; i < out.size(); ++i) {
    if (out[i].bin_lo >= out[i].bin_hi) return false;
    if (i && out[i].bin_lo != out[i - 1].bin_hi) return false;
    const u128 m = mass(bins, out[i].bin_lo, out[i].bin_hi);
    if (m == 0) return false;
    if (out[i].n != (m > (u128)~0ull ? ~0ull : (uint64_t)m)) return false;
    if (m > largest) largest = m;
  }
  // minimal: no cutting into at most `parts` ranges stays below it
  return fewest_slow(bins, lo, hi, largest - 1) > parts;
}

// every cutting of [lo, hi) (at most 16 bins) into exactly `want` ranges with entries: the smallest largest part, then the first cuts
static std::vector<uint32_t> best_slow(const std::vector<uint64_t> &bins, uint32_t lo, uint32_t hi, uint32_t want) {
  const uint32_t nb = hi - lo;
  std::vector<uint32_t> best;
  u128 best_max = 0;
  for (uint32_t mask = 0; mask < (1u << (nb - 1)); ++mask) {        // bit i: a cut after bin lo + i
    if ((uint32_t)__builtin_popcount(mask) != want - 1) continue;
    std::vector<uint32_t> cuts;
    u128 mx = 0;
    bool ok = true;
    uint32_t from = lo;
    for (uint32_t i = 0; i < nb; ++i)
      if (i == nb - 1 || (mask >> i & 1u)) {
        const u128 m = mass(bins, from, lo + i + 1);
        ok = ok && m != 0;
        if (m > mx) mx = m;
        from = lo + i + 1;
        cuts.push_back(from);
      }
    if (!ok) continue;
    if (best.empty() || mx < best_max || (mx == best_max && cuts < best)) { best = cuts; best_max = mx; }
  }
  return best;
}

static bool same_cuts(const std::vector<mfx_bin_range> &out, const std::vector<uint32_t> &cuts) {
  if (out.size() != cuts.size()) return false;
  for (size_t i = 0; i < out.size(); ++i) if (out[i].bin_hi != cuts[i]) return false;
  return true;
}

static uint64_t g_state = 0x2545F4914F6CDD1Dull;
static uint64_t rnd() { g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17; return g_state; }

int main() {
  std::vector<mfx_bin_range> out;
  // ---- empty bins, one bin
  {
    std::vector<uint64_t> z(64, 0);
    for (uint32_t parts : {1u, 2u, 64u, 4096u}) { mfx_cut_bins(z.data(), 0, 64, parts, out); check(out.empty(), "empty bins", parts, out.size(), 0); }
    mfx_cut_bins(z.data(), 5, 5, 3, out);
    check(out.empty(), "no bins", 5, 5, out.size());
    std::vector<uint64_t> one{7};
    for (uint32_t parts : {0u, 1u, 2u, 9u}) {
      mfx_cut_bins(one.data(), 0, 1, parts, out);
      check(parts == 0 ? out.empty() : (out.size() == 1 && out[0].bin_lo == 0 && out[0].bin_hi == 1 && out[0].n == 7), "one bin", parts, out.size(), 0);
    }
    std::vector<uint64_t> e1{0};
    mfx_cut_bins(e1.data(), 0, 1, 2, out);
    check(out.empty(), "one bin without entries", 2, out.size(), 0);
  }
  // ---- all mass in one bin: first, middle, last; a sub-range of the bins
  for (uint32_t where : {0u, 9u, 19u})
    for (uint32_t parts : {1u, 2u, 5u, 4096u}) {
      std::vector<uint64_t> b(20, 0);
      b[where] = 1000;
      mfx_cut_bins(b.data(), 0, 20, parts, out);
      check(cutting_ok(b, 0, 20, parts, out) && out.size() == 1 && out[0].bin_lo == 0 && out[0].bin_hi == 20, "all mass in one bin", where, parts, out.size());
      mfx_cut_bins(b.data(), 3, 17, parts, out);
      check(cutting_ok(b, 3, 17, parts, out) && out.size() == (where == 9 ? 1u : 0u), "all mass in one bin, bins 3-17", where, parts, out.size());
    }
  // ---- a heavy bin first, in the middle, last among light ones
  for (uint32_t where : {0u, 6u, 11u})
    for (uint32_t parts : {1u, 2u, 3u, 4u, 12u, 13u, 100u}) {
      std::vector<uint64_t> b(12, 10);
      b[where] = 1000;
      mfx_cut_bins(b.data(), 0, 12, parts, out);
      check(cutting_ok(b, 0, 12, parts, out) && same_cuts(out, best_slow(b, 0, 12, (uint32_t)out.size())), "heavy bin", where, parts, out.size());
    }
  // ---- parts above the non-empty bins: one range per bin with entries, the bins without entries joined to them
  {
    std::vector<uint64_t> b{0, 3, 0, 0, 5, 1, 0, 2, 0};
    for (uint32_t parts : {4u, 5u, 9u, 4096u}) {
      mfx_cut_bins(b.data(), 0, 9, parts, out);
      check(cutting_ok(b, 0, 9, parts, out) && out.size() == 4 && same_cuts(out, best_slow(b, 0, 9, 4)), "parts above the bins with entries", parts, out.size(), 0);
    }
  }
  // ---- counts near 2^64: the masses are summed in 128 bits, n saturates
  {
    std::vector<uint64_t> b{~0ull, ~0ull - 1, 1ull << 63, 1ull << 63, ~0ull, 3, ~0ull};
    for (uint32_t parts : {1u, 2u, 3u, 4u, 7u, 8u}) {
      mfx_cut_bins(b.data(), 0, 7, parts, out);
      check(cutting_ok(b, 0, 7, parts, out) && same_cuts(out, best_slow(b, 0, 7, (uint32_t)out.size())), "counts near 2^64", parts, out.size(), out.empty() ? 0 : out[0].n);
    }
  }
  // ---- small random bins against every cutting there is: the largest part minimal and, of those, the first cuts
  for (int t = 0; t < 60; ++t) {
    const uint32_t nb = 2 + (uint32_t)(rnd() % 12);
    std::vector<uint64_t> b(nb);
    for (auto &x : b) x = rnd() % 3 == 0 ? 0 : rnd() % 50;
    const uint32_t lo = (uint32_t)(rnd() % 2), parts = 1 + (uint32_t)(rnd() % (nb + 1));
    mfx_cut_bins(b.data(), lo, nb, parts, out);
    check(cutting_ok(b, lo, nb, parts, out) && (out.empty() || same_cuts(out, best_slow(b, lo, nb, (uint32_t)out.size()))), "small random bins", nb, parts, out.size());
  }
  // ---- 4096 random bins at six values of parts: flat, skewed, with stretches without entries
  for (int shape = 0; shape < 3; ++shape) {
    std::vector<uint64_t> b(4096);
    for (uint32_t i = 0; i < 4096; ++i) {
      const uint64_t r = rnd();
      b[i] = shape == 0 ? 200000 + r % 100000 : shape == 1 ? (r % 7 == 0 ? r % 100000000 : r % 1000) : ((i / 300) % 2 ? 0 : r % 5000);
    }
    for (uint32_t parts : {1u, 2u, 3u, 16u, 1000u, 4096u}) {
      mfx_cut_bins(b.data(), 0, 4096, parts, out);
      check(cutting_ok(b, 0, 4096, parts, out), "4096 random bins", shape, parts, out.size());
      mfx_cut_bins(b.data(), 1000, 3001, parts, out);
      check(cutting_ok(b, 1000, 3001, parts, out), "4096 random bins, bins 1000-3001", shape, parts, out.size());
    }
  }
  printf("%s (%d mismatches in %d cases)\n", g_bad ? "FAILED" : "OK", g_bad, g_cases);
  return g_bad ? 1 : 0;
}
