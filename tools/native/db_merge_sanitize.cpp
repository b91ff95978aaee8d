// The host side of mfx_db_merge that no device enters, under AddressSanitizer + UBSan: the window planner and the escape slicing
// (csrc/mfx_merge.h) on random directories, and the input checks of mfx_db_merge (csrc/mfx_db_merge.cpp, mfx_db_windows.cpp) on files written by mfx_db_write_flat
// and then damaged -- every such call must end in MFX_E_FORMAT (or the refusal it names) with nothing written.
//   hipcc -fsanitize=address,undefined -g -O1 -std=c++17 tools/native/db_merge_sanitize.cpp merfin_amd/csrc/mfx_db.cpp merfin_amd/csrc/mfx_db_windows.cpp \
//         merfin_amd/csrc/mfx_db_merge.cpp -Imerfin_amd/csrc -Iinclude \
//         -Lmerfin_amd -lmerfin_amd -Wl,-rpath,$PWD/merfin_amd -Wl,-rpath,/opt/rocm/lib -o /tmp/db_merge_sanitize && ASAN_OPTIONS=detect_leaks=0 /tmp/db_merge_sanitize /tmp/dbm
#include <algorithm>
#include <random>
#include <string>
#include <vector>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sys/stat.h>
#include "merfin_amd.h"
#include "mfx_merge.h"

typedef std::vector<uint64_t> Keys;
typedef std::vector<uint32_t> Vals;

static std::vector<char> slurp(const std::string &p) { std::vector<char> b; if (FILE *f = fopen(p.c_str(), "rb")) { char t[65536]; size_t n; while ((n = fread(t, 1, sizeof t, f)) > 0) b.insert(b.end(), t, t + n); fclose(f); } return b; }
static void spit(const std::string &p, const std::vector<char> &b) { if (FILE *f = fopen(p.c_str(), "wb")) { fwrite(b.data(), 1, b.size(), f); fclose(f); } }
static bool exists(const std::string &p) { struct stat st; return stat(p.c_str(), &st) == 0; }

static std::mt19937_64 rng(31);
static int bad = 0;
static std::string dir;

static void expect(bool ok, const char *what, long a = 0, long b = 0) {
  if (!ok) { printf("%s (%ld, %ld)  <-- UNEXPECTED\n", what, a, b); ++bad; }
}

// ---- the planner: the properties of tests/test_merge_plan_cpu.py on random directories
static void plan_trial(int trial) {
  const int k = 6 + (int)(rng() % 26);
  const uint64_t END = mfx_merge_end(k);
  const uint32_t n_in = 1 + (uint32_t)(rng() % 8);
  std::vector<Keys> firsts(n_in);
  std::vector<mfx_merge_input> in(n_in);
  for (uint32_t i = 0; i < n_in; ++i) {
    const size_t nb = rng() % 40;
    for (size_t b = 0; b < nb; ++b) firsts[i].push_back(rng() % END);
    std::sort(firsts[i].begin(), firsts[i].end());
    firsts[i].erase(std::unique(firsts[i].begin(), firsts[i].end()), firsts[i].end());
    const uint64_t blocks = firsts[i].size();
    in[i] = mfx_merge_input{firsts[i].data(), 1u, blocks, blocks ? (blocks - 1) * MFX_MERGE_BLOCK + 1 + rng() % MFX_MERGE_BLOCK : 0};
  }
  const uint64_t Rs[] = {0, 1, 5000, 3 * MFX_MERGE_BLOCK, 1ull << 26};
  const uint64_t R = Rs[rng() % 5];
  std::vector<mfx_merge_window> win;
  std::vector<uint64_t> blk;
  mfx_merge_plan(in.data(), n_in, k, R, win, blk);
  expect(!win.empty() && win.front().lo == 0 && win.back().hi == END, "the windows cover the key space", trial);
  expect(blk.size() == 2 * win.size() * n_in, "two block bounds per window and input", trial);
  std::vector<std::vector<char>> seen(n_in);
  for (uint32_t i = 0; i < n_in; ++i) seen[i].assign(in[i].nblocks, 0);
  for (size_t w = 0; w < win.size(); ++w) {
    expect(win[w].lo < win[w].hi, "a window is not empty", trial, (long)w);
    if (w + 1 < win.size()) expect(win[w + 1].lo == win[w].hi, "the windows follow each other", trial, (long)w);
    uint64_t pairs = 0;
    bool one_each = true;
    for (uint32_t i = 0; i < n_in; ++i) {
      const uint64_t b0 = blk[2 * (w * n_in + i)], b1 = blk[2 * (w * n_in + i) + 1];
      expect(b0 <= b1 && b1 <= in[i].nblocks, "block bounds inside the input", trial, (long)w);
      pairs += mfx_merge_block_pairs(in[i], b0, b1);
      one_each = one_each && b1 - b0 <= 1;
      for (uint64_t b = 0; b < in[i].nblocks; ++b) {
        const uint64_t b_lo = firsts[i][b], b_hi = b + 1 < in[i].nblocks ? firsts[i][b + 1] : END;
        if (b >= b0 && b < b1) seen[i][b] = 1;
        else expect(b_hi <= win[w].lo || b_lo >= win[w].hi, "a block left out holds no k-mer of the window", trial, (long)w);
      }
    }
    expect(pairs == win[w].pairs, "the window's pairs", trial, (long)w);
    if (pairs > std::max<uint64_t>(R, 1)) expect(one_each, "above R only with one block an input", trial, (long)w);
  }
  for (uint32_t i = 0; i < n_in; ++i)
    for (char s : seen[i]) expect(s != 0, "every block lies in a window", trial, (long)i);
}

// ---- the escape slicing against a plain scan
static void slice_trial(int trial) {
  Keys ek;
  const size_t n = rng() % 50;
  for (size_t i = 0; i < n; ++i) ek.push_back(rng() % 1000);
  std::sort(ek.begin(), ek.end());
  ek.erase(std::unique(ek.begin(), ek.end()), ek.end());
  const uint64_t lo = rng() % 1000, hi = lo + rng() % 1000;
  uint64_t e0 = 0, e1 = 0, w0 = 0, w1 = 0;
  mfx_merge_escape_slice(ek.data(), ek.size(), lo, hi, &e0, &e1);
  for (uint64_t x : ek) { if (x < lo) ++w0; if (x < hi) ++w1; }
  expect(e0 == w0 && e1 == w1, "the escapes of a window", trial);
  mfx_merge_escape_slice(nullptr, 0, lo, hi, &e0, &e1);
  expect(e0 == 0 && e1 == 0, "no escapes", trial);
}

// ---- the input checks: a call that must be refused with `code` before a device is touched, nothing written
static void refused(const std::vector<std::string> &ins, int code, const char *what, int op = MFX_MERGE_SUM, uint64_t lo = 0, uint64_t hi = ~0ull, const char *out_name = nullptr) {
  std::vector<const char *> p;
  for (auto &s : ins) p.push_back(s.c_str());
  const std::string out = out_name ? std::string(out_name) : dir + "/out.mfxk";
  mfx_db_merge_opts o{op, lo, hi, 0};
  mfx_db_merge_stats st;
  const int rc = mfx_db_merge(p.data(), (uint32_t)p.size(), out.c_str(), &o, &st);
  if (rc != code) printf("  got %d: %s\n", rc, mfx_last_error());
  expect(rc == code, what, rc, code);
  expect(strstr(mfx_last_error(), "hip") == nullptr, "refused before a device is asked for");
  if (!out_name) expect(!exists(out) && !exists(out + ".blocks"), "nothing written");
}

static std::string write_db(const char *name, int k, size_t n, uint32_t big_every) {
  const uint64_t mask = (1ull << (2 * k)) - 1;
  Keys keys;
  for (size_t i = 0; i < n + 16; ++i) keys.push_back(rng() & mask);
  std::sort(keys.begin(), keys.end());
  keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
  if (keys.size() > n) keys.resize(n);
  Vals vals(keys.size());
  for (size_t i = 0; i < vals.size(); ++i) vals[i] = big_every && i % big_every == 0 ? 0xffffffffu : 1u + (uint32_t)(rng() % 50);
  const std::string p = dir + "/" + name;
  if (mfx_db_write_flat(p.c_str(), k, keys.data(), vals.data(), keys.size())) { printf("writing %s: %s\n", p.c_str(), mfx_last_error()); ++bad; }
  return p;
}

int main(int argc, char **argv) {
  dir = argc > 1 ? argv[1] : "/tmp/db_merge_sanitize";
  mkdir(dir.c_str(), 0777);
  for (int t = 0; t < 400; ++t) plan_trial(t);
  for (int t = 0; t < 400; ++t) slice_trial(t);
  const std::string a = write_db("a.mfxk", 21, 3 * 4096 + 5, 37), b = write_db("b.mfxk", 21, 4097, 0), k15 = write_db("k15.mfxk", 15, 500, 0);
  refused({}, MFX_E_INVAL, "no inputs");
  refused(std::vector<std::string>(65, a), MFX_E_INVAL, "65 inputs");
  refused({a, b}, MFX_E_INVAL, "an unknown operation", 9);
  refused({a, b}, MFX_E_INVAL, "min above max", MFX_MERGE_SUM, 3, 2);
  refused({a, k15}, MFX_E_INVAL, "inputs of different k");
  refused({a, b}, MFX_E_INVAL, "the output is an input", MFX_MERGE_SUM, 0, ~0ull, b.c_str());
  refused({a, dir}, MFX_E_FORMAT, "a directory");
  refused({a, dir + "/absent"}, MFX_E_IO, "a file that is not there");
  spit(dir + "/text.txt", std::vector<char>{'A', 'C', 'G', 'T', 'A', '\t', '3', '\n'});
  refused({dir + "/text.txt"}, MFX_E_FORMAT, "text");
  setenv("MFX_FLAT_DELTA", "0", 1);
  const std::string packed = write_db("packed.mfxk", 21, 300, 0);
  unsetenv("MFX_FLAT_DELTA");
  refused({packed, a}, MFX_E_FORMAT, "a packed file");
  // damaged copies of a: every one ends in MFX_E_FORMAT before a block is read
  const std::vector<char> good = slurp(a);
  const std::string d = dir + "/damaged.mfxk";
  auto damaged = [&](const char *what, const std::vector<char> &bytes) { spit(d, bytes); refused({b, d}, MFX_E_FORMAT, what); };
  uint64_t n = 0, nesc = 0, nblocks = 0;
  memcpy(&n, good.data() + 16, 8); memcpy(&nesc, good.data() + 24, 8); memcpy(&nblocks, good.data() + 32, 8);
  expect(nblocks == 4 && nesc > 2, "the file to damage has four blocks and escapes", (long)nblocks, (long)nesc);
  for (size_t cut : {(size_t)0, (size_t)7, (size_t)31, (size_t)39, (size_t)40 + 16 * 3, good.size() - 1, good.size() - 12 * (size_t)nesc})
    damaged("a truncated file", std::vector<char>(good.begin(), good.begin() + cut));
  { auto x = good; x[0] = 'X'; spit(d, x); refused({b, d}, MFX_E_FORMAT, "bad magic"); }
  { auto x = good; uint64_t v = n + 4096; memcpy(x.data() + 16, &v, 8); damaged("a k-mer count that does not match the blocks", x); }
  { auto x = good; uint64_t v = ~0ull; memcpy(x.data() + 16, &v, 8); damaged("a k-mer count beyond the file", x); }
  { auto x = good; uint64_t v = ~0ull / 12; memcpy(x.data() + 24, &v, 8); damaged("an escape count beyond the file", x); }
  { auto x = good; uint64_t v = 5; memcpy(x.data() + 32, &v, 8); damaged("a block count that does not match", x); }
  { auto x = good; std::swap_ranges(x.begin() + 40, x.begin() + 48, x.begin() + 56); damaged("a directory that does not ascend", x); }
  { auto x = good; x[40 + 8 + 6] = 63; damaged("a key width beyond 2k bits", x); }
  { auto x = good; x[40 + 8 + 7] = 1; damaged("a count width below 2 bits", x); }
  { auto x = good; x[40 + 16 + 8] ^= 8; damaged("a block offset that does not follow the block before", x); }
  { auto x = good; uint32_t f = 8u | 4u; memcpy(x.data() + 12, &f, 4); damaged("a placed file", x); }
  {
    auto x = good;                                               // the escape list: the first two k-mers swapped, then one wider than 2k bits
    char *ek = x.data() + x.size() - 12 * nesc;
    std::swap_ranges(ek, ek + 8, ek + 8);
    damaged("an escape list that does not ascend", x);
    x = good;
    x[x.size() - 12 * nesc + 7] = 0x40;
    damaged("an escaped k-mer wider than 2k bits", x);
  }
  printf(bad ? "%d UNEXPECTED\n" : "db_merge_sanitize: all as expected\n", bad);
  return bad ? 1 : 0;
}
