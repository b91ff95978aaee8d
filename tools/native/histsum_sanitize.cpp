// The host-side sum of several slots' -hist counts images (csrc/mfx_histsum.h: the named offsets and add) under AddressSanitizer +
// UBSan, without a device and without the library: every image is a heap block of exactly MFX_HIST_WORDS words, so a word read or
// written one past either end is caught, and every sum is checked against one made the obvious way, field by field, from the slots'
// own numbers.  Identity and scattered per-contig counters, slots without contigs, an accumulator that is a slot's own image, the
// overflow count every slot reports, and counters that wrap (unsigned: defined, and it must match).
//   g++ -fsanitize=address,undefined -static-libasan -static-libubsan -g -O1 -std=c++17 tools/native/histsum_sanitize.cpp -o /tmp/histsum_sanitize && /tmp/histsum_sanitize
#include <cstdint>
#include <cstdio>
#include <memory>
#include <vector>
#include "../../merfin_amd/csrc/mfx_histsum.h"

namespace {
struct SlotCounts {                       // one slot's numbers, field by field
  std::vector<uint64_t> undr, over, ckasm, ckmissing;
  uint64_t kasm = 0, kmissing = 0, novf = 0;
  std::unique_ptr<uint32_t[]> ids;        // exactly ckasm.size() entries (none: a block of no bytes, never null); unused when the slot is the identity
};

uint64_t g_state = 0x9e3779b97f4a7c15ull;
uint64_t rnd() { g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17; return g_state; }
// small numbers, and now and then one just below 2^64, so that sums wrap
uint64_t value(bool wrap) { const uint64_t r = rnd(); return wrap && (r & 3) == 0 ? UINT64_MAX - (r >> 60) : r >> 40; }

SlotCounts make_slot(uint32_t nbins, const std::vector<uint32_t> &ids, bool wrap) {
  SlotCounts s;
  for (uint32_t i = 0; i < nbins; ++i) { s.undr.push_back(value(wrap)); s.over.push_back(value(wrap)); }
  s.kasm = value(wrap); s.kmissing = value(wrap); s.novf = value(wrap);
  s.ids.reset(new uint32_t[ids.size()]);
  for (size_t i = 0; i < ids.size(); ++i) { s.ids[i] = ids[i]; s.ckasm.push_back(value(wrap)); s.ckmissing.push_back(value(wrap)); }
  return s;
}

// the image of a slot, laid out as include/merfin_amd.h documents it (written out here, not taken from the header under test)
std::vector<uint64_t> image_of(uint32_t nbins, const SlotCounts &s) {
  const uint32_t nc = (uint32_t)s.ckasm.size();
  std::vector<uint64_t> h(2ull * nbins + 3 + 2ull * nc, 0);
  for (uint32_t i = 0; i < nbins; ++i) { h[i] = s.undr[i]; h[nbins + i] = s.over[i]; }
  h[2ull * nbins] = s.kasm; h[2ull * nbins + 1] = s.kmissing; h[2ull * nbins + 2] = s.novf;
  for (uint32_t i = 0; i < nc; ++i) { h[2ull * nbins + 3 + i] = s.ckasm[i]; h[2ull * nbins + 3 + nc + i] = s.ckmissing[i]; }
  return h;
}

int g_bad = 0;
void check(bool ok, const char *what, uint32_t nbins, uint32_t total) {
  if (!ok) { printf("MISMATCH: %s (nbins %u, %u contigs)\n", what, nbins, total); ++g_bad; }
}

// adds the slots into an accumulator (first_is_acc: slot 0's own image is the accumulator, as the drivers over replicas do) and
// compares every field with the sum over the slots
void run_case(const char *name, uint32_t nbins, uint32_t total, const std::vector<std::vector<uint32_t>> &ids_of, bool identity, bool first_is_acc, bool wrap) {
  std::vector<SlotCounts> slots;
  for (const auto &ids : ids_of) slots.push_back(make_slot(nbins, ids, wrap));
  if (MFX_HIST_WORDS(nbins, total) != 2ull * nbins + 3 + 2ull * total) check(false, "MFX_HIST_WORDS", nbins, total);
  std::vector<uint64_t> zero(MFX_HIST_WORDS(nbins, total), 0), first = first_is_acc ? image_of(nbins, slots[0]) : zero;
  uint64_t *acc = first.data();
  for (size_t d = 0; d < slots.size(); ++d) {
    const std::vector<uint64_t> own = image_of(nbins, slots[d]);
    const uint64_t *h = first_is_acc && d == 0 ? acc : own.data();
    const uint64_t n = mfx_histsum::add(acc, nbins, total, h, (uint32_t)slots[d].ckasm.size(), identity ? nullptr : slots[d].ids.get());
    check(n == slots[d].novf, "the slot's novf is returned", nbins, total);
  }
  std::vector<uint64_t> ckasm(total, 0), ckmissing(total, 0);
  uint64_t kasm = 0, kmissing = 0, novf = 0;
  for (const SlotCounts &s : slots) {
    kasm += s.kasm; kmissing += s.kmissing; novf += s.novf;
    for (size_t i = 0; i < s.ckasm.size(); ++i) { ckasm[identity ? i : s.ids[i]] += s.ckasm[i]; ckmissing[identity ? i : s.ids[i]] += s.ckmissing[i]; }
  }
  for (uint32_t i = 0; i < nbins; ++i) {
    uint64_t u = 0, o = 0;
    for (const SlotCounts &s : slots) { u += s.undr[i]; o += s.over[i]; }
    check(acc[mfx_histsum::undr(nbins) + i] == u && acc[mfx_histsum::over(nbins) + i] == o, "bins", nbins, total);
  }
  check(acc[mfx_histsum::kasm(nbins)] == kasm && acc[mfx_histsum::kmissing(nbins)] == kmissing && acc[mfx_histsum::novf(nbins)] == novf, "global counters", nbins, total);
  for (uint32_t c = 0; c < total; ++c)
    check(acc[mfx_histsum::contig_kasm(nbins) + c] == ckasm[c] && acc[mfx_histsum::contig_kmissing(nbins, total) + c] == ckmissing[c], "per-contig counters", nbins, total);
  printf("%-64s nbins %u, %u contigs, %zu slots%s\n", name, nbins, total, slots.size(), wrap ? ", wrapping" : "");
}
}  // namespace

int main() {
  for (uint32_t nbins : {1u, 5u})
    for (int wrap = 0; wrap < 2; ++wrap) {
      for (uint32_t total : {0u, 1u, 7u}) {
        std::vector<uint32_t> all(total);
        for (uint32_t c = 0; c < total; ++c) all[c] = c;
        run_case("identity, one slot", nbins, total, {all}, true, false, wrap);
        run_case("identity, three slots", nbins, total, {all, all, all}, true, false, wrap);
        run_case("identity, slot 0's image is the accumulator, two more slots", nbins, total, {all, all, all}, true, true, wrap);
        run_case("identity, slot 0's image is the accumulator and the only slot", nbins, total, {all}, true, true, wrap);
        run_case("a map that is the identity", nbins, total, {all, all}, false, false, wrap);
        run_case("slots without contigs", nbins, total, {{}, all, {}}, false, false, wrap);
      }
      run_case("one contig, in the second of two slots", nbins, 1, {{}, {0}}, false, false, wrap);
      run_case("reversed map", nbins, 7, {{6, 5, 4, 3, 2, 1, 0}}, false, false, wrap);
      run_case("three slots interleaved", nbins, 7, {{0, 3, 6}, {1, 4}, {2, 5}}, false, false, wrap);
      run_case("three slots interleaved, out of order, one without contigs", nbins, 7, {{5, 2}, {}, {6, 0, 3}, {4, 1}}, false, false, wrap);
    }
  printf(g_bad ? "FAILED: %d mismatches\n" : "OK (%d mismatches)\n", g_bad);
  return g_bad ? 1 : 0;
}
