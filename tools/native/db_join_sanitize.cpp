// The host side of mfx_db_join_* that no device enters, under AddressSanitizer + UBSan: the join kernel's tile and lane cuts and its ownership
// rule as csrc/mfx_join.h restates them for the host (mfx_join_host: the text the kernel's lanes run) on random runs and on runs with an
// equal pair on every lane and tile boundary, the window trimming (mfx_join_trim), and the input checks of mfx_db_join_* (csrc/mfx_db_join.cpp, mfx_db_windows.cpp)
// on files written by mfx_db_write_flat -- every such call must be refused with the code it names and the outputs untouched.
//   hipcc -Xarch_host -fsanitize=address,undefined -g -O1 -std=c++17 tools/native/db_join_sanitize.cpp merfin_amd/csrc/mfx_db.cpp merfin_amd/csrc/mfx_db_windows.cpp \
//         merfin_amd/csrc/mfx_db_join.cpp -Imerfin_amd/csrc -Iinclude \
//         -Lmerfin_amd -lmerfin_amd -Wl,-rpath,$PWD/merfin_amd -Wl,-rpath,/opt/rocm/lib -o /tmp/db_join_sanitize && ASAN_OPTIONS=detect_leaks=0 /tmp/db_join_sanitize /tmp/dbj
#include <algorithm>
#include <random>
#include <string>
#include <vector>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sys/stat.h>
#include "merfin_amd.h"
#include "mfx_join.h"

typedef std::vector<uint64_t> Keys;
typedef std::vector<uint32_t> Vals;

static std::mt19937_64 rng(47);
static int bad = 0;
static std::string dir;

static void expect(bool ok, const char *what, long a = 0, long b = 0) {
  if (!ok) { printf("%s (%ld, %ld)  <-- UNEXPECTED\n", what, a, b); ++bad; }
}

// ---- the walk against a plain two-pointer join: every distinct k-mer once, in ascending order, with both counts
static void join_against_plain(const Keys &ka, const Vals &va, const Keys &kb, const Vals &vb, const char *what, long tag) {
  Keys wk; Vals wr, wa;
  for (size_t i = 0, j = 0; i < ka.size() || j < kb.size();) {
    if (j == kb.size() || (i < ka.size() && ka[i] < kb[j])) { wk.push_back(ka[i]); wr.push_back(va[i]); wa.push_back(0); ++i; }
    else if (i == ka.size() || kb[j] < ka[i]) { wk.push_back(kb[j]); wr.push_back(0); wa.push_back(vb[j]); ++j; }
    else { wk.push_back(ka[i]); wr.push_back(va[i]); wa.push_back(vb[j]); ++i; ++j; }
  }
  Keys gk; Vals gr, ga;
  uint64_t calls = 0;
  mfx_join_host(ka.data(), va.data(), ka.size(), kb.data(), vb.data(), kb.size(), [&](bool have, uint64_t key, uint32_t rv, uint32_t av) {
    ++calls;
    if (have) { gk.push_back(key); gr.push_back(rv); ga.push_back(av); }
  });
  expect(calls == mfx_join_tiles(ka.size(), kb.size()) * MFX_JOIN_TILE, "every lane calls its sink MFX_JOIN_PER times a tile", tag);
  expect(gk == wk && gr == wr && ga == wa, what, tag, (long)gk.size() - (long)wk.size());
}

static void random_trial(int trial) {
  const size_t sizes[] = {0, 1, 7, 8, 9, 2047, 2048, 2049, 4096, 3 * 4096 + 17};
  const size_t la = sizes[rng() % 10], lb = sizes[rng() % 10];
  const uint64_t space = 1 + (la + lb) * (1 + rng() % 4);       // dense to sparse: many to few keys in both
  Keys ka, kb;
  for (uint64_t x = 0; x < space * 2 && (ka.size() < la || kb.size() < lb); ++x) {
    const unsigned r = (unsigned)(rng() % 4);
    if ((r & 1u) && ka.size() < la) ka.push_back(x);
    if ((r & 2u) && kb.size() < lb) kb.push_back(x);
  }
  Vals va(ka.size()), vb(kb.size());
  for (auto &v : va) v = 1u + (uint32_t)(rng() % 1000);
  for (auto &v : vb) v = 1u + (uint32_t)(rng() % 5);
  join_against_plain(ka, va, kb, vb, "a random join", trial);
}

// An equal pair on every multiple of `grain` in merged order, shifted by `shift`: merged position p holds a key of both runs (its read record;
// the asm twin at p + 1) when (p + shift) % grain == grain - 1, so the boundary falls between the twins (shift 0), just behind the pair
// (shift 1: the asm twin is the last position of the share) or just in front of it; the positions between alternate read-only / asm-only.
static void boundary_world(uint32_t grain, uint32_t shift, size_t total) {
  Keys ka, kb;
  uint64_t key = 10;
  for (size_t p = 0; p < total;) {
    if ((p + shift) % grain == grain - 1) { ka.push_back(key); kb.push_back(key); p += 2; }
    else { ((p / 3) % 2 ? ka : kb).push_back(key); p += 1; }
    key += 1 + rng() % 3;
  }
  Vals va(ka.size()), vb(kb.size());
  for (size_t i = 0; i < va.size(); ++i) va[i] = 100u + (uint32_t)i;
  for (size_t i = 0; i < vb.size(); ++i) vb[i] = 1u + (uint32_t)(i % 7);
  join_against_plain(ka, va, kb, vb, "an equal pair on every boundary", (long)grain * 10000 + shift);
}

// ---- the trimming of a window's run
static void trim_trial(int trial) {
  const uint64_t nblocks = rng() % 5;
  std::vector<uint32_t> below(nblocks, 0), above(nblocks, 0);
  uint64_t len = nblocks ? (nblocks - 1) * 4096 + 1 + rng() % 4096 : 0;
  const uint64_t last = nblocks ? len - (nblocks - 1) * 4096 : 0;
  if (nblocks) {
    below[0] = (uint32_t)(rng() % (nblocks == 1 ? last + 1 : 4097));
    above[nblocks - 1] = (uint32_t)(rng() % (last + 1 - (nblocks == 1 ? below[0] : 0)));
  }
  uint64_t off = 0, n = 0;
  const uint64_t at = rng() % 1000;
  expect(mfx_join_trim(at, len, below.data(), above.data(), nblocks, &off, &n), "a prefix and a suffix are trimmed", trial);
  expect(off == at + (nblocks ? below[0] : 0) && n == len - (nblocks ? below[0] + above[nblocks - 1] : 0), "the dense run", trial);
  if (nblocks >= 2) {
    std::vector<uint32_t> b2 = below, a2 = above;
    b2[1] = 1;
    expect(!mfx_join_trim(at, len, b2.data(), above.data(), nblocks, &off, &n), "records under the window in a block that is not the first", trial);
    a2[0] = 1;
    expect(!mfx_join_trim(at, len, below.data(), a2.data(), nblocks, &off, &n), "records over the window in a block that is not the last", trial);
  }
  if (nblocks) {
    std::vector<uint32_t> b2 = below;
    b2[0] = (uint32_t)len + 1;
    expect(!mfx_join_trim(at, len, b2.data(), above.data(), nblocks, &off, &n), "more trimmed than the blocks hold", trial);
  }
}

// ---- the input checks: calls that must be refused with `code` before a device is touched, the outputs as they were
static void refused(const char *r, const char *a, int code, const char *what, const char *text, uint32_t copies = 4, uint32_t max_mult = 100) {
  mfx_db_join_opts o;
  memset(&o, 0, sizeof(o));
  o.maxV = ~0ull; o.peak = 20.0; o.copies = copies; o.max_mult = max_mult;
  double t[64], u[64];
  for (int i = 0; i < 64; ++i) t[i] = u[i] = -1.0;
  std::vector<uint64_t> img((size_t)(copies + 2) * (max_mult + 1), 77);
  uint64_t n = 77;
  mfx_db_join_stats st;
  int rc = mfx_db_join_completeness(r, a, &o, t, u, &st);
  if (rc != code || (text && !strstr(mfx_last_error(), text))) { printf("  completeness got %d: %s\n", rc, mfx_last_error()); ++bad; }
  expect(strstr(mfx_last_error(), "hip") == nullptr, "refused before a device is asked for");
  rc = mfx_db_join_spectrum(r, a, &o, img.data(), &n, &st);
  if (rc != code || (text && !strstr(mfx_last_error(), text))) { printf("  spectrum got %d: %s\n", rc, mfx_last_error()); ++bad; }
  expect(rc == code, what, rc, code);
  bool same = n == 77;
  for (int i = 0; i < 64; ++i) same = same && t[i] == -1.0 && u[i] == -1.0;
  for (uint64_t x : img) same = same && x == 77;
  expect(same, "the outputs of a refused call are untouched");
}

static std::string write_db(const char *name, int k, size_t n) {
  const uint64_t mask = k < 32 ? (1ull << (2 * k)) - 1 : ~0ull;
  Keys keys;
  for (size_t i = 0; i < n + 16; ++i) keys.push_back(rng() & mask);
  std::sort(keys.begin(), keys.end());
  keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
  if (keys.size() > n) keys.resize(n);
  Vals vals(keys.size());
  for (auto &v : vals) v = 1u + (uint32_t)(rng() % 50);
  const std::string p = dir + "/" + name;
  if (mfx_db_write_flat(p.c_str(), k, keys.data(), vals.data(), keys.size())) { printf("writing %s: %s\n", p.c_str(), mfx_last_error()); ++bad; }
  return p;
}

int main(int argc, char **argv) {
  dir = argc > 1 ? argv[1] : "/tmp/db_join_sanitize";
  mkdir(dir.c_str(), 0777);
  for (int t = 0; t < 300; ++t) random_trial(t);
  for (uint32_t grain : {MFX_JOIN_PER, MFX_JOIN_TILE})
    for (uint32_t shift : {0u, 1u, 2u, grain - 1})
      boundary_world(grain, shift, 3 * MFX_JOIN_TILE + 5 * MFX_JOIN_PER + 3);
  for (int t = 0; t < 400; ++t) trim_trial(t);
  const std::string a = write_db("a.mfxk", 21, 3 * 4096 + 5), b = write_db("b.mfxk", 21, 4097), k15 = write_db("k15.mfxk", 15, 500);
  refused(a.c_str(), k15.c_str(), MFX_E_INVAL, "inputs of different k", "the inputs are of one k");
  refused(nullptr, b.c_str(), MFX_E_INVAL, "a null path", "null argument");
  refused(a.c_str(), dir.c_str(), MFX_E_FORMAT, "a directory", nullptr);
  refused((dir + "/absent").c_str(), b.c_str(), MFX_E_IO, "a file that is not there", "does not exist");
  {
    FILE *f = fopen((dir + "/text.txt").c_str(), "w");
    if (f) { fputs("ACGTA\t3\n", f); fclose(f); }
    refused(a.c_str(), (dir + "/text.txt").c_str(), MFX_E_FORMAT, "text", "run `merfin -convert` first");
  }
  setenv("MFX_FLAT_DELTA", "0", 1);
  const std::string packed = write_db("packed.mfxk", 21, 300);
  unsetenv("MFX_FLAT_DELTA");
  refused(packed.c_str(), a.c_str(), MFX_E_FORMAT, "a packed file", "run `merfin -convert` first");
  {
    std::vector<char> x;
    if (FILE *f = fopen(a.c_str(), "rb")) { char t[65536]; size_t n; while ((n = fread(t, 1, sizeof t, f)) > 0) x.insert(x.end(), t, t + n); fclose(f); }
    uint32_t fl = 8u | 4u;
    memcpy(x.data() + 12, &fl, 4);
    if (FILE *f = fopen((dir + "/placed.mfxk").c_str(), "wb")) { fwrite(x.data(), 1, x.size(), f); fclose(f); }
    refused(b.c_str(), (dir + "/placed.mfxk").c_str(), MFX_E_FORMAT, "a placed file", "placed");      // (the flag alone: the header check names it first)
  }
  {                                                              // the spectrum's bounds: the completeness call does not look at them
    mfx_db_join_opts o;
    memset(&o, 0, sizeof(o));
    o.maxV = ~0ull;
    uint64_t img[8 * 5], n = 0;
    for (uint32_t copies : {0u, 7u}) {
      o.copies = copies; o.max_mult = 4;
      expect(mfx_db_join_spectrum(a.c_str(), b.c_str(), &o, img, &n, nullptr) == MFX_E_INVAL && strstr(mfx_last_error(), "copies ="), "copies out of bounds", copies);
    }
    for (uint32_t mm : {3u, 65537u}) {
      o.copies = 1; o.max_mult = mm;
      expect(mfx_db_join_spectrum(a.c_str(), b.c_str(), &o, img, &n, nullptr) == MFX_E_INVAL && strstr(mfx_last_error(), "max_mult ="), "max_mult out of bounds", mm);
    }
    o.copies = 4; o.max_mult = 100;
    expect(mfx_db_join_spectrum(a.c_str(), b.c_str(), &o, nullptr, &n, nullptr) == MFX_E_INVAL, "a null image");
    double t[64];
    expect(mfx_db_join_completeness(a.c_str(), b.c_str(), &o, t, nullptr, nullptr) == MFX_E_INVAL, "a null sum");
  }
  printf(bad ? "%d UNEXPECTED\n" : "db_join_sanitize: all as expected\n", bad);
  return bad ? 1 : 0;
}
