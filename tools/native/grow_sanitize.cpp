// grow_sanitize.cpp -- the plain host arithmetic of csrc/mfx_grow.h under AddressSanitizer + UBSan (tests/test_grow_cpu.py builds and
// runs it): the growth rule of the claiming read counter's table and the grouping of mfx_index_write_db's bins into key ranges, each
// checked against a definition written out the slow way.  Prints one line per case and exits non-zero on a mismatch.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../merfin_amd/csrc/mfx_grow.h"

static int g_bad = 0, g_cases = 0;
static void check(bool ok, const char *what, unsigned long long a, unsigned long long b, unsigned long long c) {
  ++g_cases;
  printf("%s %s (%llu, %llu, %llu)\n", ok ? "ok      " : "MISMATCH", what, a, b, c);
  if (!ok) ++g_bad;
}

// ---- the bounds, in long double on small numbers where 0.7 x slots and 0.35 x slots are exact tenths / twentieths
static void growth_cases() {
  // around 0.7: slots = 8192 -> 5734.4: 5734 fits, 5735 does not, however the sum is split
  const uint64_t slots = 8192;
  for (uint64_t total : {0ull, 1ull, 5733ull, 5734ull, 5735ull, 8192ull, 100000ull})
    for (int split = 0; split < 4; ++split) {
      const uint64_t d = split == 0 ? total : split == 1 ? 0 : total / 3, p = split == 1 ? total : split == 2 ? total / 3 : 0, B = total - d - p;
      check(mfx_grow_fits(d, p, B, slots) == (total <= 5734), "fits, 8192 slots", d, p, B);
    }
  // exact at a multiple of ten: 10 slots -> 7
  check(mfx_grow_fits(3, 2, 2, 10), "fits, 7 of 10", 3, 2, 2);
  check(!mfx_grow_fits(3, 2, 3, 10), "fits, 8 of 10", 3, 2, 3);
  // no overflow at the top of the range: 2^35 slots, 2^34 positions in a batch, counts near 2^64
  check(mfx_grow_fits(1ull << 34, 1ull << 31, 1ull << 32, 1ull << 35), "fits, large", 1ull << 34, 1ull << 31, 1ull << 32);
  check(!mfx_grow_fits(1ull << 34, 0, 1ull << 33, 1ull << 35), "fits, large, 0.75", 1ull << 34, 0, 1ull << 33);
  check(!mfx_grow_fits(~0ull, ~0ull, ~0ull, 1ull << 35), "fits, all ones", ~0ull, ~0ull, ~0ull);
  check(!mfx_grow_fits(0, 0, 1, 0), "fits, no slots", 0, 0, 1);

  // around 0.35: 1024 lines of 8 slots; 16384 slots -> 5734.4, 32768 -> 11468.8, 65536 -> 22937.6
  struct { uint64_t d, B, want; } g[] = {
    {0, 1, 2048}, {0, 5734, 2048}, {0, 5735, 4096}, {5734, 0, 2048}, {5000, 735, 4096}, {11468, 0, 4096}, {11468, 1, 8192},
    {22937, 0, 8192}, {22938, 0, 16384}, {40000, 69, 16384}, {0, 0, 2048},
  };
  for (const auto &c : g) check(mfx_grow_lines(c.d, c.B, 1024, 8, (1ull << 32) - 16) == c.want, "grow from 1024 lines", c.d, c.B, c.want);
  // the result is a power-of-two multiple of the lines it started from, also where those are no power of two
  for (uint64_t nl : {1024ull, 1500ull, 99999ull})
    for (uint64_t need : {1ull, 3000ull, 123456ull, 99999999ull}) {
      const uint64_t r = mfx_grow_lines(need, 0, nl, 8, (1ull << 32) - 16);
      uint64_t m = r / nl;
      bool ok = r != 0 && r % nl == 0 && m >= 2 && (m & (m - 1)) == 0 && 20 * need <= 7 * r * 8;
      if (ok && m > 2) ok = 20 * need > 7 * (r / 2) * 8;            // and the smallest such
      check(ok, "grow, multiple", nl, need, r);
    }
  // no table below the line limit: 0, not a wrapped number
  check(mfx_grow_lines(1ull << 40, 0, 1024, 8, (1ull << 32) - 16) == 0, "grow, beyond the limit", 1ull << 40, 0, 0);
  check(mfx_grow_lines(~0ull, ~0ull, 1ull << 31, 8, (1ull << 32) - 16) == 0, "grow, all ones", ~0ull, ~0ull, 0);
  check(mfx_grow_lines(5, 5, 0, 8, 100) == 0, "grow, no lines", 5, 5, 0);
  // a bound that FAILS the 0.7 test always finds a table that passes it with room: after growth distinct + B <= 0.35 x slots
  for (uint64_t d = 0; d < 200000; d += 7919)
    for (uint64_t B : {45ull, 97ull, 1000ull, 5000ull, 1ull << 20}) {
      const uint64_t r = mfx_grow_lines(d, B, 1024, 8, (1ull << 32) - 16);
      check(r != 0 && mfx_grow_fits(d, 0, B, r * 8) && mfx_grow_fits(2 * d, 0, 2 * B, r * 8), "grow, then fits twice over", d, B, r);
    }
}

// ---- ranges: no range empty, ascending, every non-empty bin in exactly one, at most R entries unless a single bin
static void range_case(const char *what, const std::vector<uint64_t> &bins, uint64_t R) {
  std::vector<mfx_bin_range> out;
  mfx_group_bins(bins.data(), (uint32_t)bins.size(), R, out);
  bool ok = true;
  uint64_t total = 0, got = 0;
  for (uint64_t b : bins) total += b;
  uint32_t prev_hi = 0;
  const uint64_t Reff = R ? R : 1;
  for (size_t i = 0; i < out.size(); ++i) {
    const auto &r = out[i];
    uint64_t n = 0;
    uint32_t nonempty = 0;
    ok = ok && r.bin_lo < r.bin_hi && r.bin_hi <= bins.size() && r.bin_lo >= prev_hi;
    if (!ok) break;
    for (uint32_t b = prev_hi; b < r.bin_lo; ++b) ok = ok && bins[b] == 0;           // only empty bins are skipped
    for (uint32_t b = r.bin_lo; b < r.bin_hi; ++b) { n += bins[b]; nonempty += bins[b] != 0; }
    ok = ok && n == r.n && n != 0 && (n <= Reff || nonempty == 1) && bins[r.bin_lo] != 0 && bins[r.bin_hi - 1] != 0;
    // greedy: the next non-empty bin would not have fitted
    if (i + 1 < out.size()) ok = ok && (bins[out[i + 1].bin_lo] > Reff || n > Reff - bins[out[i + 1].bin_lo]);
    got += n;
    prev_hi = r.bin_hi;
  }
  for (uint32_t b = prev_hi; b < bins.size(); ++b) ok = ok && bins[b] == 0;
  check(ok && got == total, what, bins.size(), R, out.size());
}

static void range_cases() {
  range_case("ranges, no bins", {}, 10);
  range_case("ranges, all empty", std::vector<uint64_t>(64, 0), 10);
  range_case("ranges, zeros between", {0, 0, 3, 0, 0, 4, 0, 5, 0, 0}, 7);
  range_case("ranges, zeros between, R = 1", {0, 0, 3, 0, 0, 4, 0, 5, 0, 0}, 1);
  range_case("ranges, one bin larger than R", {2, 2, 50, 2, 2}, 5);
  range_case("ranges, first bin larger than R", {50, 1, 1}, 5);
  range_case("ranges, last bin larger than R", {1, 1, 50}, 5);
  range_case("ranges, every bin larger than R", {9, 9, 9, 9}, 1);
  range_case("ranges, exact fill", {5, 5, 5, 5, 5, 5}, 10);
  range_case("ranges, last range short", {5, 5, 5, 5, 5}, 10);
  range_case("ranges, one range", {1, 2, 3, 4}, 1ull << 28);
  range_case("ranges, R = 0 taken as 1", {1, 0, 2}, 0);
  range_case("ranges, counts near 2^64", {~0ull - 3, 2, 5}, ~0ull - 1);
  range_case("ranges, R = 2^64 - 1", {1ull << 62, 1ull << 62, 1ull << 62}, ~0ull);
  std::vector<uint64_t> big(4096);
  uint64_t x = 88172645463325252ull;
  for (auto &b : big) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; b = (x % 5 == 0) ? 0 : x % 1000; }
  for (uint64_t R : {1ull, 17ull, 999ull, 1000ull, 5000ull, 1ull << 28}) range_case("ranges, 4096 random bins", big, R);
}

int main() {
  growth_cases();
  range_cases();
  printf("%s (%d mismatches, %d cases)\n", g_bad ? "FAILED" : "OK", g_bad, g_cases);
  return g_bad ? 1 : 0;
}
