// The streamed database writer on the host (csrc/mfx_db.cpp: mfx_db_writer_open_streamed, mfx_db_writer_append_sorted, _info, _close,
// _abort) under AddressSanitizer + UBSan, without a device: the cases of tests/test_db_writer_stream.py -- sizes around a block, appends
// of 1 / 4095 / 4096 / 4097 k-mers, every kind of block, refused appends, abort, a spool that cannot be created.  Every file must equal
// what mfx_db_write_flat writes for the same arrays.
//   hipcc -fsanitize=address,undefined -g -O1 -std=c++17 tools/native/db_stream_sanitize.cpp merfin_amd/csrc/mfx_db.cpp -Imerfin_amd/csrc -Iinclude \
//         -Lmerfin_amd -lmerfin_amd -Wl,-rpath,$PWD/merfin_amd -Wl,-rpath,/opt/rocm/lib -o /tmp/db_stream_sanitize && ASAN_OPTIONS=detect_leaks=0 /tmp/db_stream_sanitize /tmp/dbs
#include <algorithm>
#include <random>
#include <string>
#include <vector>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sys/stat.h>
#include "merfin_amd.h"

typedef std::vector<uint64_t> Keys;
typedef std::vector<uint32_t> Vals;

static std::vector<char> slurp(const std::string &p) { std::vector<char> b; if (FILE *f = fopen(p.c_str(), "rb")) { char t[65536]; size_t n; while ((n = fread(t, 1, sizeof t, f)) > 0) b.insert(b.end(), t, t + n); fclose(f); } return b; }
static bool exists(const std::string &p) { struct stat st; return stat(p.c_str(), &st) == 0; }

static std::mt19937_64 rng(29);
static int bad = 0;
static std::string dir;

static void expect(bool ok, const char *what, int k, size_t n, size_t piece) {
  if (!ok) { printf("k=%d n=%lu piece=%lu: %s  <-- UNEXPECTED\n", k, (unsigned long)n, (unsigned long)piece, what); ++bad; }
}

static Keys random_keys(int k, size_t n) {
  const uint64_t mask = (1ull << (2 * k)) - 1;
  if (n > mask) n = (size_t)mask + 1;
  Keys keys;
  while (keys.size() < n) {
    for (size_t i = keys.size(); i < n + 16; ++i) keys.push_back(rng() & mask);
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
  }
  keys.resize(n);
  return keys;
}

// the arrays through a streamed writer in appends of `piece` k-mers, compared with the plain writer's file
static void one(int k, const Keys &keys, const Vals &vals, size_t piece) {
  const size_t n = keys.size();
  const std::string plain = dir + "/plain.mfxk", out = dir + "/stream.mfxk", spool = out + ".blocks";
  remove(out.c_str());
  expect(mfx_db_write_flat(plain.c_str(), k, keys.data(), vals.data(), n) == MFX_OK, "write_flat failed", k, n, piece);
  mfx_db_writer *w = mfx_db_writer_open_streamed(out.c_str(), k);
  if (!w) { expect(false, mfx_last_error(), k, n, piece); return; }
  expect(exists(spool) && !exists(out), "before close: a spool, nothing at path", k, n, piece);
  for (size_t o = 0; o < n; o += piece)
    expect(mfx_db_writer_append_sorted(w, keys.data() + o, vals.data() + o, std::min(piece, n - o)) == MFX_OK, "append_sorted failed", k, n, piece);
  uint64_t nk = 0, nb = 0, ne = 0, sb = 0, hb = 0;
  expect(mfx_db_writer_info(w, &nk, &nb, &ne, &sb, &hb) == MFX_OK && nk == n && nb == n / 4096 && hb == 16 * nb + 12 * ne + 12 * (n % 4096), "info", k, n, piece);
  struct stat st;
  expect(stat(spool.c_str(), &st) == 0 && (uint64_t)st.st_size == sb, "spool_bytes is the spool's size", k, n, piece);
  uint64_t closed = ~0ull;
  expect(mfx_db_writer_close(w, &closed) == MFX_OK && closed == n, "close failed", k, n, piece);
  expect(!exists(spool), "the spool stayed after close", k, n, piece);
  expect(slurp(out) == slurp(plain), "the bytes differ from the plain writer's", k, n, piece);
}

static Vals mixed(size_t n) {
  Vals v(n);
  for (size_t i = 0; i < n; ++i) v[i] = i % 401 == 0 ? 0xffffffffu : i % 977 == 7 ? (1u << 22) - 1 : i % 53 == 0 ? 1 + (uint32_t)(rng() % (1u << 21)) : 1 + (uint32_t)(rng() % 59);
  return v;
}

int main(int argc, char **argv) {
  dir = argc > 1 ? argv[1] : "/tmp";
  mkdir(dir.c_str(), 0777);
  for (int k : {7, 21, 31}) {
    for (size_t n : {(size_t)0, (size_t)1, (size_t)4095, (size_t)4096, (size_t)4097, (size_t)3 * 4096}) {
      const Keys keys = random_keys(k, n);
      const Vals vals = mixed(keys.size());
      for (size_t piece : {(size_t)1, (size_t)4095, (size_t)4096, (size_t)4097, std::max<size_t>(n, 1)}) one(k, keys, vals, piece);
    }
    // the kinds of block
    const Keys keys = random_keys(k, 2 * 4096 + 1234);
    const size_t n = keys.size();
    std::vector<Vals> kinds;
    Vals v(n);
    for (auto &x : v) x = 1 + (uint32_t)(rng() % 2);
    kinds.push_back(v);                                        // vb = 2
    for (auto &x : v) x = 1 + (uint32_t)(rng() % ((1u << 22) - 2));
    v[0] = (1u << 22) - 2;
    kinds.push_back(v);                                        // vb = 22, nothing escapes
    for (size_t i = 0; i < n; ++i) v[i] = i % 5 == 0 ? (1u << 22) - 1 : i % 7 == 1 ? 0xffffffffu : 1 + (uint32_t)(rng() % 8);
    kinds.push_back(v);                                        // escapes
    std::fill(v.begin(), v.end(), 1u);
    for (int i = 0; i < 6; ++i) v[(size_t)(rng() % 4096)] = 1000000u;
    kinds.push_back(v);                                        // escaping is cheaper
    std::fill(v.begin(), v.end(), 1u);
    for (size_t i = 0; i < 4096; i += 2) v[i] = 1000000u;
    kinds.push_back(v);                                        // widening is cheaper
    for (auto &x : v) x = 1 + (uint32_t)(rng() % 2);
    for (size_t i = 0; i < 128; ++i) v[i * 32 + 5] = 20u;
    kinds.push_back(v);                                        // a cost tie: 4096 x 2 + 96 x 128 == 4096 x 5
    for (const Vals &kv : kinds)
      for (size_t piece : {n, (size_t)4097, (size_t)1000}) one(k, keys, kv, piece);
  }
  {                                                            // every 7-mer: kb = 1; the ends of the 31-mers: kb = 62
    Keys all(16384);
    for (size_t i = 0; i < all.size(); ++i) all[i] = i;
    one(7, all, mixed(all.size()), 5000);
    one(31, Keys{0, (1ull << 62) - 1}, Vals{3, 0xffffffffu}, 1);
    one(31, Keys{0, (1ull << 62) - 1}, Vals{3, 0xffffffffu}, 2);
  }
  // refused appends add nothing, for both kinds of writer; abort; a spool that cannot be created
  for (int streamed = 0; streamed < 2; ++streamed) {
    const int k = 21;
    const Keys keys = random_keys(k, 3 * 4096 + 500);
    const Vals vals = mixed(keys.size());
    const size_t n = keys.size(), a = 4096 + 100, b = 3 * 4096 + 7;
    const std::string plain = dir + "/plain.mfxk", out = dir + "/refused.mfxk";
    remove(out.c_str());
    mfx_db_write_flat(plain.c_str(), k, keys.data(), vals.data(), n);
    mfx_db_writer *w = streamed ? mfx_db_writer_open_streamed(out.c_str(), k) : mfx_db_writer_open(out.c_str(), k);
    if (!w) { expect(false, mfx_last_error(), k, n, 0); continue; }
    expect(mfx_db_writer_append_sorted(w, keys.data(), vals.data(), a) == MFX_OK, "append", k, n, a);
    uint64_t i0[5], i1[5];
    mfx_db_writer_info(w, &i0[0], &i0[1], &i0[2], &i0[3], &i0[4]);
    expect(mfx_db_writer_append_sorted(w, keys.data(), vals.data(), a) == MFX_E_INVAL, "a too-low append was taken", k, n, a);
    expect(mfx_db_writer_append_sorted(w, keys.data() + a - 1, vals.data() + a - 1, b - a + 1) == MFX_E_INVAL, "an append from the last k-mer was taken", k, n, a);
    Keys dup(keys.begin() + a, keys.begin() + b);
    dup[4096 + 50] = dup[4096 + 49];
    expect(mfx_db_writer_append_sorted(w, dup.data(), vals.data() + a, dup.size()) == MFX_E_INVAL, "a repeated k-mer was taken", k, n, a);
    std::swap(dup[3], dup[4]);
    expect(mfx_db_writer_append_sorted(w, dup.data(), vals.data() + a, dup.size()) == MFX_E_INVAL, "unsorted k-mers were taken", k, n, a);
    mfx_db_writer_info(w, &i1[0], &i1[1], &i1[2], &i1[3], &i1[4]);
    expect(memcmp(i0, i1, sizeof i0) == 0, "a refused append changed the writer", k, n, a);
    expect(mfx_db_writer_append_sorted(w, keys.data() + a, vals.data() + a, b - a) == MFX_OK, "append", k, n, b);
    expect(mfx_db_writer_append_sorted(w, nullptr, nullptr, 0) == MFX_OK, "append of nothing", k, n, b);
    expect(mfx_db_writer_append_sorted(w, keys.data() + b, vals.data() + b, n - b) == MFX_OK, "append", k, n, n);
    expect(mfx_db_writer_close(w, nullptr) == MFX_OK, "close", k, n, n);
    expect(slurp(out) == slurp(plain) && !exists(out + ".blocks"), "the bytes after refused appends", k, n, n);
    remove(out.c_str());
    w = streamed ? mfx_db_writer_open_streamed(out.c_str(), k) : mfx_db_writer_open(out.c_str(), k);
    if (w) {
      mfx_db_writer_append_sorted(w, keys.data(), vals.data(), n);
      mfx_db_writer_abort(w);
    }
    expect(w && !exists(out) && !exists(out + ".blocks"), "abort left a file", k, n, n);
  }
  expect(mfx_db_writer_open_streamed((dir + "/no/such/dir.mfxk").c_str(), 21) == nullptr && strstr(mfx_last_error(), "cannot create the spool"), "open without a directory", 21, 0, 0);
  expect(mfx_db_writer_open_streamed((dir + "/k32.mfxk").c_str(), 32) == nullptr && !exists(dir + "/k32.mfxk.blocks"), "open with k = 32", 32, 0, 0);
  printf("done, unexpected: %d\n", bad);
  return bad != 0;
}
