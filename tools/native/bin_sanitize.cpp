// The host arithmetic of -bin (csrc/mfx_bin.h: the cut of records into batches and pieces, the first piece of every tile, the fold of
// piece counts into records, the class rule) under AddressSanitizer + UBSan, over the length grid of tests/test_bin_cpu.py and over
// random lengths, with the invariants that test asserts -- and the kernel's piece arithmetic (mfx_kernels.hip, mfx_bin_kernel: the
// start bits of a tile, their prefix counts, the piece of a position) restated for the host and held against a walk over the pieces.
// No device, no library.
//   g++ -fsanitize=address,undefined -static-libasan -static-libubsan -g -O1 -std=c++17 -Wall -Werror -Imerfin_amd/csrc -Iinclude
//       tools/native/bin_sanitize.cpp -o /tmp/bin_sanitize && /tmp/bin_sanitize
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
#include "mfx_bin.h"

static int bad = 0, cases = 0;
#define CHECK(c, ...) do { if (!(c)) { if (bad++ < 20) { fprintf(stderr, "FAIL %s:%d: %s: ", __FILE__, __LINE__, #c); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)

struct Batch { std::vector<mfx_bin_piece> pieces; uint64_t npos; std::vector<uint8_t> bytes; };

// the records as texts of their own letter each, so that a batch's bytes say which record every base came from
static std::vector<Batch> cut(const std::vector<uint64_t> &lens, uint64_t k, uint64_t cap) {
  std::vector<std::vector<char>> text(lens.size());
  std::vector<const char *> ptr(lens.size());
  for (size_t i = 0; i < lens.size(); ++i) { text[i].assign((size_t)lens[i] + 1, (char)('a' + i % 26)); ptr[i] = text[i].data(); }
  mfx_batch b;
  b.cap = cap;
  b.bytes.resize((size_t)cap + 32);
  std::vector<Batch> out;
  std::vector<mfx_bin_piece> open;
  uint64_t reads = 0, bases = 0;
  auto flush = [&]() {
    if (b.used) out.push_back(Batch{open, b.used, std::vector<uint8_t>(b.bytes.begin(), b.bytes.begin() + (size_t)b.used)});
    open.clear();
    b.used = 0;
    return 0;
  };
  const int rc = mfx_batch_records(b, k, ptr.data(), lens.data(), (uint64_t)lens.size(), reads, bases, [](uint64_t) { return -1; }, flush,
                                   [&](uint64_t i, uint64_t first, uint64_t len, bool last) { open.push_back(mfx_bin_piece{i, first, len, last}); });
  flush();
  uint64_t sum = 0;
  for (uint64_t l : lens) sum += l;
  CHECK(rc == 0 && reads == lens.size() && bases == sum, "rc %d", rc);
  // the plan alone (no text) cuts the same pieces
  mfx_batch pb;
  pb.cap = cap;
  std::vector<mfx_bin_piece> plan;
  std::vector<uint64_t> plan_batch;
  uint64_t nb = 0, r2 = 0, b2 = 0;
  mfx_batch_records(pb, k, nullptr, lens.data(), (uint64_t)lens.size(), r2, b2, [](uint64_t) { return -1; }, [&]() { if (pb.used) ++nb; pb.used = 0; return 0; },
                    [&](uint64_t i, uint64_t first, uint64_t len, bool last) { plan.push_back(mfx_bin_piece{i, first, len, last}); plan_batch.push_back(nb); });
  size_t at = 0;
  for (size_t bi = 0; bi < out.size(); ++bi)
    for (const mfx_bin_piece &p : out[bi].pieces) {
      CHECK(at < plan.size() && plan_batch[at] == bi && plan[at].record == p.record && plan[at].first == p.first && plan[at].len == p.len && plan[at].last == p.last,
            "plan and cut differ at piece %zu", at);
      ++at;
    }
  CHECK(at == plan.size(), "%zu pieces cut, %zu planned", at, plan.size());
  return out;
}

// the piece of every position as mfx_bin_kernel finds it, against a walk over the pieces
static void check_kernel_arithmetic(const Batch &B, uint64_t k) {
  const uint64_t T = MFX_BIN_TILE, np = B.pieces.size(), ntiles = (B.npos + T - 1) / T;
  std::vector<uint64_t> tile_first((size_t)ntiles);
  mfx_bin_tile_first(B.pieces.data(), np, B.npos, tile_first.data());
  std::vector<int64_t> owner((size_t)B.npos, -1);                // the piece that holds the position's k-mer whole
  for (uint64_t q = 0; q < np; ++q)
    for (uint64_t p = B.pieces[q].first; p + k <= B.pieces[q].first + B.pieces[q].len; ++p) owner[(size_t)p] = (int64_t)q;
  for (uint64_t t = 0; t < ntiles; ++t) {
    const uint64_t pos0 = t * T, piece0 = tile_first[(size_t)t];
    CHECK(piece0 <= np, "tile %lu", (unsigned long)t);
    const uint32_t base = (piece0 < np && B.pieces[(size_t)piece0].first < pos0) ? 1u : 0u;
    uint64_t bits[64] = {0};
    for (uint64_t q = piece0 + base; q < np; ++q) {
      const uint64_t s = B.pieces[(size_t)q].first;
      if (s >= pos0 + T) break;
      CHECK(s >= pos0, "piece %lu starts in front of its tile", (unsigned long)q);
      bits[(s - pos0) >> 6] |= 1ull << ((s - pos0) & 63);
    }
    uint32_t pre[65];
    pre[0] = 0;
    for (int w = 0; w < 64; ++w) pre[w + 1] = pre[w] + (uint32_t)__builtin_popcountll(bits[w]);
    uint32_t before = 0;
    for (uint64_t p = 0; p < T && pos0 + p < B.npos; ++p) {
      const uint64_t upto = bits[p >> 6] & (~0ull >> (63 - (p & 63)));
      const uint32_t started = base + pre[p >> 6] + (uint32_t)__builtin_popcountll(upto);
      const uint32_t win = started ? started - 1 : 0;
      CHECK(win >= before, "the piece decreases at %lu", (unsigned long)(pos0 + p));
      before = win;
      if (owner[(size_t)(pos0 + p)] >= 0) CHECK(piece0 + win == (uint64_t)owner[(size_t)(pos0 + p)], "position %lu: piece %lu, the walk says %ld", (unsigned long)(pos0 + p),
                                                (unsigned long)(piece0 + win), (long)owner[(size_t)(pos0 + p)]);
      CHECK(piece0 + win < np || owner[(size_t)(pos0 + p)] < 0, "position %lu", (unsigned long)(pos0 + p));
    }
  }
}

static void check(const std::vector<uint64_t> &lens, uint64_t k, uint64_t cap) {
  ++cases;
  const std::vector<Batch> bs = cut(lens, k, cap);
  std::vector<uint64_t> kmers(lens.size(), 0);
  std::vector<int64_t> first_batch(lens.size(), -1), last_batch(lens.size(), -1);
  std::vector<uint32_t> recs(lens.size() * 4, 0);
  for (size_t bi = 0; bi < bs.size(); ++bi) {
    const Batch &B = bs[bi];
    CHECK(B.npos <= cap && !B.pieces.empty(), "batch %zu", bi);
    uint64_t end = 0;
    std::vector<uint32_t> counts;
    for (size_t q = 0; q < B.pieces.size(); ++q) {
      const mfx_bin_piece &p = B.pieces[q];
      CHECK(p.len >= k, "a piece of %lu bases", (unsigned long)p.len);                     // no piece is shorter than k
      CHECK(q == 0 ? p.first == 0 : p.first == end + 1, "pieces ascend, one separator apart");
      end = p.first + p.len;
      CHECK(end <= B.npos, "a piece beyond its batch");
      for (uint64_t i = p.first; i < end; ++i) CHECK(B.bytes[(size_t)i] == (uint8_t)('a' + p.record % 26), "byte %lu is not of record %lu", (unsigned long)i, (unsigned long)p.record);
      if (end < B.npos) CHECK(B.bytes[(size_t)end] == 'N', "no separator behind piece %zu", q);
      if (q) CHECK(p.record > B.pieces[q - 1].record && B.pieces[q - 1].last, "two pieces of one record in a batch");
      kmers[(size_t)p.record] += mfx_bin_piece_kmers(p.len, k);
      if (first_batch[(size_t)p.record] < 0) first_batch[(size_t)p.record] = (int64_t)bi;
      CHECK(last_batch[(size_t)p.record] < 0 || last_batch[(size_t)p.record] == (int64_t)bi - 1, "pieces of record %lu skip a batch", (unsigned long)p.record);
      last_batch[(size_t)p.record] = (int64_t)bi;
      const uint32_t n = (uint32_t)mfx_bin_piece_kmers(p.len, k);
      counts.insert(counts.end(), {n, n / 3, n / 5, n / 7});
    }
    mfx_bin_fold(B.pieces.data(), B.pieces.size(), counts.data(), [&](uint64_t r) { return &recs[(size_t)r * 4]; });
    check_kernel_arithmetic(B, k);
  }
  for (size_t r = 0; r < lens.size(); ++r) {
    const uint64_t want = lens[r] >= k ? lens[r] - k + 1 : 0;
    CHECK(kmers[r] == want && recs[r * 4] == want, "record %zu of %lu bases: %lu k-mers in its pieces", r, (unsigned long)lens[r], (unsigned long)kmers[r]);
    CHECK((first_batch[r] < 0) == (lens[r] < k), "record %zu", r);
  }
}

static int plain_class(uint32_t a, uint32_t b, uint64_t na, uint64_t nb, uint32_t ratio, uint32_t hits) {
  typedef unsigned __int128 u;
  const u NA = na ? na : 1, NB = nb ? nb : 1;
  const bool enough = (uint64_t)a + b >= hits;
  if (enough && (u)a * NB * 1000 > (u)b * NA * ratio) return 0;
  if (enough && (u)b * NA * 1000 > (u)a * NB * ratio) return 1;
  return 2;
}

int main() {
  std::mt19937_64 rng(20240611);
  for (uint64_t k : {6ull, 15ull, 21ull, 31ull}) {
    const std::vector<uint64_t> grid = {0, k - 1, k, k + 1, 63, 64, 65, 4095, 4096, 4097, 2 * 4096 + 5};
    for (uint64_t cap : {2 * k + 2, (uint64_t)100, (uint64_t)4096, (uint64_t)10000, (uint64_t)(1 << 16)}) {
      if (cap < mfx_batch_bases_min((int)k)) continue;
      check(grid, k, cap);
      check(std::vector<uint64_t>(grid.rbegin(), grid.rend()), k, cap);
      for (uint64_t a : grid) {
        check({a}, k, cap);
        for (uint64_t b : {(uint64_t)0, k - 1, k, k + 1, (uint64_t)65}) check({a, b, a}, k, cap);
      }
      check(std::vector<uint64_t>(700, k), k, cap);               // reads of exactly k, back to back: MFX_TILE / (k + 1) pieces a tile
      check({cap - 1 - k, k, 50}, k, cap);                        // a record that ends exactly at the batch's end: no separator
      check({0, 1, k - 1, 2, 0}, k, cap);                         // all short
      check({}, k, cap);
      for (int rep = 0; rep < 6; ++rep) {
        std::vector<uint64_t> lens(200);
        for (uint64_t &l : lens) l = rng() % 10 < 3 ? rng() % (k + 3) : rng() % (3 * cap < 20000 ? 3 * cap : 20000);
        check(lens, k, cap);
      }
    }
  }
  // the class rule against its statement, 128-bit products included
  const uint32_t big = 0xffffffffu;
  const uint64_t top = (1ull << 62) - 1;
  const std::vector<uint32_t> vals = {0, 1, 2, 3, 5, 10, 1000, 2499, 2500, 2501, big - 1, big};
  const std::vector<uint64_t> norms = {0, 1, 3, 7, 100, 250, top - 1, top};
  for (uint32_t a : vals) for (uint32_t b : vals) for (uint64_t na : norms) for (uint64_t nb : norms)
    for (uint32_t ratio : {1000u, 1001u, 2500u, 4000000000u}) for (uint32_t hits : {0u, 1u, 3u, 11u, big}) {
      const int got = mfx_bin_class(a, b, na, nb, ratio, hits), want = plain_class(a, b, na, nb, ratio, hits);
      CHECK(got == want && !(a == b && na == nb && got != 2) && !(a == 0 && b == 0 && got != 2), "class(%u, %u, %lu, %lu, %u, %u) = %d, want %d", a, b, (unsigned long)na,
            (unsigned long)nb, ratio, hits, got, want);
      // never both: with the roles swapped the classes swap
      const int sw = mfx_bin_class(b, a, nb, na, ratio, hits);
      CHECK(sw == (got == 2 ? 2 : 1 - got), "swapped roles");
    }
  printf("%d cases, %d failures\n", cases, bad);
  return bad ? 1 : 0;
}
