// Pass 2 of -phase as csrc/mfx_phase.h restates it for the host (mfx_phase_planes_host: the word arithmetic the plane kernels of
// csrc/mfx_phase.hip run -- the carried marker and its operator, run starts per 64-bit word, marker ranks, long and short runs, block
// openings, block sums) under AddressSanitizer + UBSan, against a walk over the markers one by one: markers on every word and tile edge,
// runs and opposite runs over empty tiles, contigs that touch, empty and short contigs, contigs with only short runs, alternating markers,
// intrusions of S and S + 1 markers and of spans R and R + 1, random planes -- each at every -switches and -range value of the tests.
// No device, no library.
//   g++ -fsanitize=address,undefined -static-libasan -static-libubsan -g -O1 -std=c++17 -Wall -Werror -Imerfin_amd/csrc -Iinclude
//       tools/native/phase_sanitize.cpp -o /tmp/phase_sanitize && /tmp/phase_sanitize
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>
#include "mfx_phase.h"

static int bad = 0, cases = 0;
static const uint64_t K = 21;

struct World {
  std::vector<uint64_t> lens;
  std::vector<std::vector<int8_t>> m;                         // per contig, per position: -1 no marker, 0 A, 1 B
  void add(uint64_t len) { lens.push_back(len); m.push_back(std::vector<int8_t>(len, -1)); }
  void set(uint32_t c, uint64_t p, int hap) { m[c][p] = (int8_t)hap; }
  uint64_t stretch(uint32_t c, uint64_t p, int hap, uint64_t n, uint64_t step = 3) { for (uint64_t i = 0; i < n; ++i) set(c, p + i * step, hap); return p + n * step; }
};

struct Run { int hap; uint64_t first, last, n; };

// marker by marker: the definition (include/merfin_amd.h, at mfx_phase_block)
static std::vector<mfx_phase_block> plain(const World &w, uint64_t S, uint64_t R) {
  std::vector<mfx_phase_block> out;
  for (uint32_t c = 0; c < w.lens.size(); ++c) {
    std::vector<Run> runs;
    for (uint64_t p = 0; p < w.lens[c]; ++p) {
      const int h = w.m[c][p];
      if (h < 0) continue;
      if (!runs.empty() && runs.back().hap == h) { runs.back().last = p; runs.back().n++; }
      else runs.push_back(Run{h, p, p, 1});
    }
    int last_long = -1;
    std::vector<std::vector<Run>> blocks;
    for (const Run &r : runs) {
      const bool is_long = !(r.n <= S && r.last - r.first + K <= R);
      if (blocks.empty() || (is_long && last_long >= 0 && last_long != r.hap)) blocks.push_back({});
      blocks.back().push_back(r);
      if (is_long) last_long = r.hap;
    }
    for (const std::vector<Run> &b : blocks) {
      uint64_t n[2] = {0, 0}, nr[2] = {0, 0};
      int hap = -1;
      for (const Run &r : b) {
        n[r.hap] += r.n;
        nr[r.hap]++;
        if (!(r.n <= S && r.last - r.first + K <= R)) hap = r.hap;
      }
      if (hap < 0) hap = n[1] > n[0] ? 1 : 0;
      out.push_back(mfx_phase_block{c, (uint32_t)hap, b.front().first, b.back().last + 1, n[hap], n[1 - hap], nr[1 - hap]});
    }
  }
  return out;
}

static void check_at(const World &w, const char *what, uint64_t S, uint64_t R) {
  std::vector<uint64_t> tile_start(w.lens.size() + 1, 0);
  for (size_t c = 0; c < w.lens.size(); ++c) tile_start[c + 1] = tile_start[c] + (w.lens[c] + MFX_RG_TILE - 1) / MFX_RG_TILE;
  const uint64_t ntiles = tile_start.back(), nw = ntiles * MFX_RG_WORDS;
  std::vector<uint32_t> tile_contig((size_t)ntiles);
  std::vector<uint64_t> planes((size_t)(2 * nw), 0);
  for (size_t c = 0; c < w.lens.size(); ++c) {
    for (uint64_t t = tile_start[c]; t < tile_start[c + 1]; ++t) tile_contig[t] = (uint32_t)c;
    for (uint64_t p = 0; p < w.lens[c]; ++p)
      if (w.m[c][p] >= 0) planes[(uint64_t)w.m[c][p] * nw + tile_start[c] * MFX_RG_WORDS + p / 64] |= 1ull << (p % 64);
  }
  std::vector<mfx_phase_block> got;
  mfx_phase_planes_host(planes.data(), ntiles, tile_start.data(), tile_contig.data(), K, S, R, got);
  const std::vector<mfx_phase_block> want = plain(w, S, R);
  bool same = got.size() == want.size();
  for (size_t i = 0; same && i < got.size(); ++i)
    same = got[i].contig == want[i].contig && got[i].hap == want[i].hap && got[i].start == want[i].start && got[i].end == want[i].end &&
           got[i].n_hap == want[i].n_hap && got[i].n_switch == want[i].n_switch && got[i].n_switch_runs == want[i].n_switch_runs;
  ++cases;
  if (!same) { printf("MISMATCH %s: switches %lu, range %lu: %zu records, %zu expected\n", what, (unsigned long)S, (unsigned long)R, got.size(), want.size()); ++bad; }
}

static const uint64_t SW[] = {0, 1, 3, 100}, RG[] = {0, K, 64, 5000, 1000000};

static void check(const World &w, const char *what) {
  for (uint64_t S : SW)
    for (uint64_t R : RG) check_at(w, what, S, R);
}

int main() {
  {                                                           // the word arithmetic itself
    const uint64_t a5 = mfx_ph_mark(5, 0), b9 = mfx_ph_mark(9, 1);
    const bool ok = mfx_ph_mark_pos(b9) == 9 && mfx_ph_mark_hap(b9) == 1 && mfx_ph_mark_hap(a5) == 0 && mfx_ph_join(a5, 0) == a5 && mfx_ph_join(a5, b9) == b9 &&
                    mfx_ph_join(a5, MFX_PH_RESET) == MFX_PH_RESET && mfx_ph_join(MFX_PH_RESET | a5, b9) == (MFX_PH_RESET | b9) &&
                    mfx_ph_join(mfx_ph_join(a5, MFX_PH_RESET), b9) == mfx_ph_join(a5, mfx_ph_join(MFX_PH_RESET, b9)) &&
                    mfx_ph_word_last(0, 0, 64) == 0 && mfx_ph_word_last(1ull << 63, 1ull << 63, 64) == mfx_ph_mark(127, 1) &&
                    mfx_ph_starts(0x7ull, 0x2ull, 0) == 0x7ull && mfx_ph_starts(0x7ull, 0x0ull, a5) == 0 && mfx_ph_starts(0x7ull, 0x0ull, b9) == 1ull &&
                    mfx_ph_starts(1ull << 63 | 1ull, 1ull << 63, a5) == 1ull << 63 && mfx_ph_before(0x5ull, 0x1ull, 2, 64, a5) == mfx_ph_mark(64, 1) &&
                    mfx_ph_before(0x4ull, 0, 2, 64, a5) == a5 && mfx_ph_below(~0ull, 63) == 63 && mfx_ph_long(1, 10, 11, K, 0, 100) && !mfx_ph_long(1, 10, 11, K, 1, K) &&
                    mfx_ph_long(2, 10, 12, K, 2, K) && mfx_ph_head(true, false, 0, 0) && !mfx_ph_head(false, true, 0, 0) && !mfx_ph_head(false, true, 0, 1) &&
                    mfx_ph_head(false, true, 0, 2) && !mfx_ph_head(false, false, 0, 2) && mfx_ph_block_hap(2, 9, 1) == 1 && mfx_ph_block_hap(0, 3, 3) == 0 &&
                    mfx_ph_block_hap(0, 3, 4) == 1 && mfx_ph_other_runs(5, 0, 0) == 2 && mfx_ph_other_runs(5, 0, 1) == 3 && mfx_ph_other_runs(1, 1, 1) == 0;
    ++cases;
    if (!ok) { printf("MISMATCH the arithmetic of a word\n"); ++bad; }
  }
  {
    World w;                                                  // markers on every edge, the last position of a contig
    w.add(3 * 4096 + 77);
    int h = 0;
    for (uint64_t p : {0ull, 63ull, 64ull, 127ull, 128ull, 255ull, 256ull, 4095ull, 4096ull, 8191ull, 8192ull, 3ull * 4096 + 76}) { w.set(0, p, h & 1); h += (p % 3 == 0); }
    check(w, "edges");
  }
  {
    World w;                                                  // a run over 3 empty tiles, opposite runs separated by 3 empty tiles, a tile + one position
    w.add(10 * 4096); w.add(4097);
    w.set(0, 100, 0); w.set(0, 200, 0); w.set(0, 4 * 4096 + 5, 0); w.set(0, 4 * 4096 + 100, 1); w.set(0, 8 * 4096 + 50, 0); w.set(0, 9 * 4096 + 4095, 0);
    w.set(1, 0, 0); w.set(1, 4096, 1);
    check(w, "empty tiles");
  }
  {
    World w;                                                  // contigs that touch; empty and short contigs and one without a marker between
    w.add(4096); w.add(0); w.add(10); w.add(8192); w.add(5000); w.add(4097); w.add(1);
    w.set(0, 4000, 0); w.set(0, 4095, 0); w.set(3, 0, 0); w.set(3, 1, 1); w.set(3, 8191, 1); w.set(5, 4096, 0); w.set(6, 0, 1);
    check(w, "contigs that touch");
  }
  {
    World w;                                                  // only short runs: majority and tie; alternating markers; every position a marker
    w.add(600); w.add(600); w.add(200 * 7 + 50); w.add(9000);
    for (uint64_t i = 0; i < 5; ++i) w.set(0, 10 + 40 * i, (int)(1 - (i & 1)));
    for (uint64_t i = 0; i < 4; ++i) w.set(1, 10 + 40 * i, (int)(1 - (i & 1)));
    for (uint64_t i = 0; i < 200; ++i) w.set(2, 5 + 7 * i, (int)(i & 1));
    for (uint64_t p = 0; p < 9000; ++p) w.set(3, p, (int)((p / 130) & 1));
    check(w, "short, alternating, full");
  }
  for (uint64_t S : SW)
    for (uint64_t R : RG) {                                   // shapes made for one grid point
      World w;
      w.add(40 * (S + 8));                                    // intrusions of S and S + 1 markers
      uint64_t p = w.stretch(0, 7, 0, S + 5);
      for (uint64_t n : {S, S + 1}) { p = w.stretch(0, p, 1, n); p = w.stretch(0, p, 0, S + 5); }
      w.add(40 * (S + 8));                                    // leading and trailing short runs; short runs between long runs of opposite haplotypes
      p = w.stretch(1, 2, 1, 1); p = w.stretch(1, p, 0, S + 5); p = w.stretch(1, p, 1, 1);
      p = w.stretch(1, p + 9, 1, S + 5); p = w.stretch(1, p, 0, 1); p = w.stretch(1, p, 1, 1); p = w.stretch(1, p, 0, S + 5);
      if (S >= 2 && R >= K + S - 1) {                         // an intrusion of S markers whose span is exactly R and R + 1
        w.add(2 * R + 40 * (S + 8));
        p = w.stretch(2, 3, 0, S + 5);
        for (uint64_t span : {R, R + 1}) {
          for (uint64_t i = 0; i + 1 < S; ++i) w.set(2, p + i, 1);
          w.set(2, p + span - K, 1);
          p = w.stretch(2, p + span - K + 1, 0, S + 5);
        }
      }
      check_at(w, "intrusions and spans", S, R);
    }
  {
    World w;
    check(w, "no contig");
    w.add(0);
    check(w, "an empty contig");
  }
  std::mt19937_64 rng(13);
  for (int trial = 0; trial < 12; ++trial) {                  // random planes, dense to sparse, haplotypes in stretches
    World w;
    const int nc = 1 + (int)(rng() % 4);
    for (int c = 0; c < nc; ++c) {
      const uint64_t lens[] = {0, 1, 63, 64, 65, 4095, 4096, 4097, 9000, 5 * 4096};
      w.add(lens[rng() % 10]);
      const uint64_t den = 1 + rng() % 300, flip = 2 + rng() % 40;
      int hap = 0;
      for (uint64_t p = 0; p < w.lens.back(); ++p) {
        if (rng() % flip == 0) hap ^= 1;
        if (rng() % den == 0) w.m.back()[p] = (int8_t)hap;
      }
    }
    check(w, ("random " + std::to_string(trial)).c_str());
  }
  printf("%s (%d mismatches, %d cases)\n", bad ? "FAILED" : "OK", bad, cases);
  return bad ? 1 : 0;
}
