// The steps of -regions between its two passes as csrc/mfx_regions.h restates them for the host (mfx_regions_planes_host: the word
// arithmetic the plane kernels of csrc/mfx_regions.hip run -- run starts and ends per 64-bit word, the neighbour bit, count, scan, scatter,
// the head rule, the filter, the records' order) under AddressSanitizer + UBSan, against a walk over the positions one by one: single bits
// on every word and tile edge, full words, alternating bits, runs over three words, contigs whose planes touch, empty and short contigs,
// random planes -- each at every gap and filter value of the tests.  No device, no library.
//   g++ -fsanitize=address,undefined -static-libasan -static-libubsan -g -O1 -std=c++17 -Wall -Werror -Imerfin_amd/csrc -Iinclude
//       tools/native/regions_sanitize.cpp -o /tmp/regions_sanitize && /tmp/regions_sanitize
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>
#include "mfx_regions.h"

typedef std::vector<std::vector<uint8_t>> Masks;             // [class][position] of one contig

static int bad = 0, cases = 0;

struct World {
  std::vector<uint64_t> lens;
  std::vector<Masks> m;                                       // per contig
  void add(uint64_t len) { lens.push_back(len); m.push_back(Masks(3, std::vector<uint8_t>(len, 0))); }
  void set(uint32_t c, uint32_t cls, uint64_t a, uint64_t b) { for (uint64_t p = a; p < b; ++p) m[c][cls][p] = 1; }
};

// position by position: the definition (include/merfin_amd.h, at mfx_region)
static std::vector<mfx_region> plain(const World &w, uint64_t gap, uint64_t min_kmers) {
  std::vector<mfx_region> out;
  for (uint32_t c = 0; c < w.lens.size(); ++c) {
    std::vector<mfx_region> mine;
    for (uint32_t cls = 0; cls < 3; ++cls) {
      std::vector<mfx_region> regs;
      const std::vector<uint8_t> &x = w.m[c][cls];
      for (uint64_t p = 0; p < x.size(); ++p) {
        if (!x[p]) continue;
        if (!regs.empty() && p - regs.back().end <= gap) {       // (end is exclusive: p - end positions lie between)
          regs.back().end = p + 1;
          regs.back().n_kmers++;
        } else {
          mfx_region r{c, cls, p, p + 1, 1, 0, 0, 0.0};
          regs.push_back(r);
        }
      }
      for (const mfx_region &r : regs) if (r.n_kmers >= min_kmers) mine.push_back(r);
    }
    for (size_t i = 1; i < mine.size(); ++i)                  // by start, then class (three sorted lists: an insertion sort will do)
      for (size_t j = i; j > 0 && (mine[j].start < mine[j - 1].start || (mine[j].start == mine[j - 1].start && mine[j].cls < mine[j - 1].cls)); --j) std::swap(mine[j], mine[j - 1]);
    out.insert(out.end(), mine.begin(), mine.end());
  }
  return out;
}

static void check(const World &w, const char *what) {
  std::vector<uint64_t> tile_start(w.lens.size() + 1, 0);
  for (size_t c = 0; c < w.lens.size(); ++c) tile_start[c + 1] = tile_start[c] + (w.lens[c] + MFX_RG_TILE - 1) / MFX_RG_TILE;
  const uint64_t ntiles = tile_start.back(), nw = ntiles * MFX_RG_WORDS;
  std::vector<uint32_t> tile_contig((size_t)ntiles);
  std::vector<uint64_t> planes((size_t)(3 * nw), 0);
  for (size_t c = 0; c < w.lens.size(); ++c) {
    for (uint64_t t = tile_start[c]; t < tile_start[c + 1]; ++t) tile_contig[t] = (uint32_t)c;
    for (uint32_t cls = 0; cls < 3; ++cls)
      for (uint64_t p = 0; p < w.lens[c]; ++p)
        if (w.m[c][cls][p]) planes[cls * nw + tile_start[c] * MFX_RG_WORDS + p / 64] |= 1ull << (p % 64);
  }
  const uint64_t gaps[] = {0, 1, 20, 64, 4096, 1000000}, mins[] = {0, 1, 21, 1000};
  for (uint64_t gap : gaps)
    for (uint64_t mk : mins) {
      std::vector<mfx_region> got;
      mfx_regions_planes_host(planes.data(), ntiles, tile_start.data(), tile_contig.data(), gap, mk, got);
      const std::vector<mfx_region> want = plain(w, gap, mk);
      bool same = got.size() == want.size();
      for (size_t i = 0; same && i < got.size(); ++i)
        same = got[i].contig == want[i].contig && got[i].cls == want[i].cls && got[i].start == want[i].start && got[i].end == want[i].end &&
               got[i].n_kmers == want[i].n_kmers && got[i].sum_readK == 0 && got[i].sum_asmK == 0 && got[i].ext_kstar == 0.0;
      ++cases;
      if (!same) { printf("MISMATCH %s: gap %lu, min %lu: %zu records, %zu expected\n", what, (unsigned long)gap, (unsigned long)mk, got.size(), want.size()); ++bad; }
    }
}

int main() {
  {                                                           // the word arithmetic itself
    const bool ok = mfx_rg_starts(0x8000000000000001ull, 0) == 0x8000000000000001ull && mfx_rg_starts(1ull, 1) == 0 && mfx_rg_starts(~0ull, 0) == 1ull &&
                    mfx_rg_ends(~0ull, 0) == 1ull << 63 && mfx_rg_ends(~0ull, 1) == 0 && mfx_rg_ends(0x5ull, 0) == 0x5ull &&
                    mfx_rg_head(true, 0, 0, 0, 0, 0) && !mfx_rg_head(false, 2, 10, 2, 11, 1) && mfx_rg_head(false, 2, 10, 2, 12, 1) && mfx_rg_head(false, 1, 10, 2, 0, ~0ull);
    ++cases;
    if (!ok) { printf("MISMATCH the masks of a word\n"); ++bad; }
  }
  {
    World w;                                                  // single bits on every edge, the last bit of a contig
    w.add(3 * 4096 + 77);
    for (uint64_t p : {0ull, 63ull, 64ull, 255ull, 256ull, 4095ull, 4096ull, 8191ull, 8192ull, 3ull * 4096 + 76}) w.set(0, (uint32_t)(p % 3), p, p + 1);
    check(w, "single bits");
  }
  {
    World w;                                                  // full words, runs over three words, runs over the wave, round and tile edges
    w.add(2 * 4096 + 5);
    w.set(0, 0, 64, 128); w.set(0, 0, 192, 384); w.set(0, 1, 60, 70); w.set(0, 1, 250, 262); w.set(0, 1, 4090, 4100); w.set(0, 2, 100, 300);
    w.set(0, 2, 8190, 8197);
    check(w, "words and edges");
  }
  {
    World w;                                                  // alternating bits over a tile edge; everything set
    w.add(9000);
    for (uint64_t p = 0; p < 9000; p += 2) w.set(0, 0, p, p + 1);
    w.set(0, 1, 0, 9000);
    check(w, "alternating and full");
  }
  {
    World w;                                                  // contigs whose planes touch: one ends flagged, the next starts flagged; empty and short contigs between
    w.add(4096); w.add(8192); w.add(0); w.add(10); w.add(4097); w.add(1);
    w.set(0, 0, 4000, 4096); w.set(1, 0, 0, 50); w.set(1, 0, 8100, 8192); w.set(3, 0, 0, 10); w.set(4, 0, 0, 3); w.set(4, 0, 4096, 4097); w.set(5, 0, 0, 1);
    w.set(0, 2, 4095, 4096); w.set(1, 2, 0, 1);
    check(w, "contigs that touch");
  }
  {
    World w;
    check(w, "no contig");
    w.add(0);
    check(w, "an empty contig");
  }
  std::mt19937_64 rng(11);
  for (int trial = 0; trial < 12; ++trial) {                  // random planes, dense to sparse
    World w;
    const int nc = 1 + (int)(rng() % 4);
    for (int c = 0; c < nc; ++c) {
      const uint64_t lens[] = {0, 1, 63, 64, 65, 4095, 4096, 4097, 9000, 12288};
      w.add(lens[rng() % 10]);
      const uint64_t den = 2 + rng() % 200;
      for (uint32_t cls = 0; cls < 3; ++cls) {
        uint8_t on = 0;
        for (uint64_t p = 0; p < w.lens.back(); ++p) { if (rng() % den == 0) on ^= 1; w.m.back()[cls][p] = on; }
      }
    }
    check(w, ("random " + std::to_string(trial)).c_str());
  }
  printf("%s (%d mismatches, %d cases)\n", bad ? "FAILED" : "OK", bad, cases);
  return bad ? 1 : 0;
}
