// The arena of a batch of the variant modes (csrc/mfx_var_arena.h: the pieces mfx_score_paths, mfx_score_paths_trv and mfx_claim_paths_batch
// carve out of one device allocation) without a device: the layout over a host block of exactly the size it asks for, so AddressSanitizer
// sees a piece that reaches past the end.  Every piece starts on a 256-byte boundary, holds what its array needs, overlaps no other, and the
// total is the sum the two callers computed before the layout had a file of its own -- those formulas are written out below, piece by piece.
//   g++ -fsanitize=address,undefined -std=c++17 -I merfin_amd/csrc tools/native/var_arena_check.cpp
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "mfx_var_arena.h"

static int bad = 0;
#define CHECK(x) do { if (!(x)) { printf("MISMATCH %s:%d: %s\n", __FILE__, __LINE__, #x); ++bad; } } while (0)

static uint64_t r256(uint64_t bytes) { return (bytes + 255) & ~255ull; }

// the scoring form's sum: text, readV, asmV, stats, off, len, nv, voff, cfirst, gt, vidx, vlen, numM, totdk, cl, var, al, win, alt, np, status
static uint64_t score_sum(const mfx_var_sizes &z) {
  const uint64_t total = z.total, NP = z.npaths, NV = z.nvals;
  const uint64_t text_bytes = ((total + 4096 - 1) / 4096 + 2) * 4096 + 256;
  return r256(text_bytes) + r256(total * 4) + r256(total * 4) + r256(16) + r256(NP * 8) + r256(NP * 4) + r256(NP * 4) + r256(NP * 8) + r256(NP * 8) +
         r256((NV ? NV : 1) * 4) + r256((NV ? NV : 1) * 4) + r256((NV ? NV : 1) * 4) + r256(NP * 4) + r256((z.need_dk ? NP : 1) * 8) + r256(z.ncl * 56) +
         r256(z.nvar * 16) + r256(z.nal * 16) + r256(z.win_bytes) + r256(z.al_bytes) + r256(z.ncl * 4) + r256(z.ncl * 4);
}

// the claim form's: text, geometry, off, len, nv, voff, cfirst, gt, vidx, vlen, cl, var, al, win, alt, np, status
static uint64_t claim_sum(const mfx_var_sizes &z) {
  const uint64_t total = z.total, NP = z.npaths, NV = z.nvals, ncl = z.ncl;
  const uint64_t ntiles = (total + 4096 - 1) / 4096;
  const uint64_t text_bytes = (ntiles + 2) * 4096 + 256;
  return r256(text_bytes) + r256(4 * 8) + r256((NP ? NP : 1) * 8) + r256((NP ? NP : 1) * 4) + r256((NP ? NP : 1) * 4) + r256((NP ? NP : 1) * 8) + r256((NP ? NP : 1) * 8) +
         r256((NV ? NV : 1) * 4) + r256((NV ? NV : 1) * 4) + r256((NV ? NV : 1) * 4) + r256((ncl ? ncl : 1) * 56) + r256(z.nvar * 16 + 8) + r256(z.nal * 16 + 8) +
         r256(z.win_bytes + 8) + r256(z.al_bytes + 8) + r256((ncl ? ncl : 1) * 4) + r256((ncl ? ncl : 1) * 4);
}

static void check(const char *name, const mfx_var_sizes &z) {
  const uint64_t need = mfx_var_arena_lay(z, nullptr, nullptr);
  CHECK(need == (z.claim ? claim_sum(z) : score_sum(z)));
  CHECK(need % 256 == 0 && need > 0);
  uint8_t *base = static_cast<uint8_t *>(aligned_alloc(256, need));
  mfx_var_arena A;
  CHECK(mfx_var_arena_lay(z, base, &A) == need);
  CHECK(A.text_bytes == ((z.total + 4095) / 4096 + 2) * 4096 + 256);
  struct Piece { const char *what; void *p; uint64_t bytes; };      // bytes: what the kernels and copies of the callers touch
  std::vector<Piece> P = {{"text", A.text, A.text_bytes}, {"off", A.off, z.npaths * 8}, {"len", A.len, z.npaths * 4}, {"nv", A.nv, z.npaths * 4},
                          {"voff", A.voff, z.npaths * 8}, {"cfirst", A.cfirst, z.npaths * 8}, {"gt", A.gt, z.nvals * 4}, {"vidx", A.vidx, z.nvals * 4},
                          {"vlen", A.vlen, z.nvals * 4}, {"cl", A.cl, z.ncl * sizeof(mfx_trv_cluster)}, {"var", A.var, z.nvar * sizeof(mfx_trv_variant)},
                          {"al", A.al, z.nal * sizeof(mfx_trv_allele)}, {"win", A.win, z.win_bytes}, {"alt", A.alt, z.al_bytes}, {"np", A.np, z.ncl * 4},
                          {"status", A.status, z.ncl * 4}};
  if (z.claim) {
    P.push_back({"geo", A.geo, 4 * 8});
    CHECK(!A.readV && !A.asmV && !A.stats && !A.numM && !A.totdk);
  } else {
    P.push_back({"readV", A.readV, z.total * 4});
    P.push_back({"asmV", A.asmV, z.total * 4});
    P.push_back({"stats", A.stats, 2 * 8});
    P.push_back({"numM", A.numM, z.npaths * 4});
    P.push_back({"totdk", A.totdk, (z.need_dk ? z.npaths : 0) * 8});
    CHECK(!A.geo);
  }
  std::sort(P.begin(), P.end(), [](const Piece &a, const Piece &b) { return a.p != b.p ? a.p < b.p : a.bytes < b.bytes; });      // (an empty piece lies where the next one starts)
  for (size_t i = 0; i < P.size(); ++i) {
    uint8_t *p = static_cast<uint8_t *>(P[i].p);
    uint8_t *next = i + 1 < P.size() ? static_cast<uint8_t *>(P[i + 1].p) : base + need;
    const bool ok = p >= base && (p - base) % 256 == 0 && p + P[i].bytes <= next;
    if (!ok) { printf("MISMATCH %s: piece %s at %ld, %lu bytes, next piece at %ld\n", name, P[i].what, (long)(p - base), (unsigned long)P[i].bytes, (long)(next - base)); ++bad; }
    else memset(p, (int)i + 1, P[i].bytes);                        // (a piece beyond the block: AddressSanitizer stops here)
  }
  for (size_t i = 0; i < P.size(); ++i)                             // ... and no piece's bytes were written by another's fill
    for (uint64_t j = 0; j < P[i].bytes; j += std::max<uint64_t>(1, P[i].bytes - 1)) CHECK(static_cast<uint8_t *>(P[i].p)[j] == (uint8_t)(i + 1));
  free(base);
}

int main() {
  int cases = 0;
  auto run = [&](const char *name, mfx_var_sizes z) {
    for (const uint64_t total : {z.total, (uint64_t)0, (uint64_t)1, (uint64_t)4095, (uint64_t)4096, (uint64_t)4097}) {
      z.total = total;
      check(name, z);
    }
    printf("case %s\n", name);
    ++cases;
  };
  auto sizes = [](uint64_t total, uint64_t np, uint64_t nv, uint64_t ncl, uint64_t nvar, uint64_t nal, uint64_t win, uint64_t alt, bool need_dk, bool claim) {
    mfx_var_sizes z;
    z.total = total; z.npaths = np; z.nvals = nv; z.ncl = ncl; z.nvar = nvar; z.nal = nal; z.win_bytes = win; z.al_bytes = alt; z.need_dk = need_dk; z.claim = claim;
    return z;
  };
  for (const bool dk : {false, true}) {
    run(dk ? "empty batch, need_dk" : "empty batch", sizes(0, 0, 0, 0, 0, 0, 0, 0, dk, false));
    run(dk ? "host part only, need_dk" : "host part only", sizes(70001, 1037, 2991, 0, 0, 0, 0, 0, dk, false));
    run(dk ? "device part only, need_dk" : "device part only", sizes(50000, 640, 1900, 33, 71, 150, 4001, 333, dk, false));
    run(dk ? "both parts, need_dk" : "both parts", sizes(123457, 1037 + 640, 2991 + 1900, 33, 71, 150, 4001, 333, dk, false));
    run(dk ? "nvals == 0, need_dk" : "nvals == 0", sizes(999, 7, 0, 0, 0, 0, 0, 0, dk, false));
    run(dk ? "row_cap == 0, need_dk" : "row_cap == 0", sizes(5000, 64 + 3, 5, 3, 3, 6, 200, 12, dk, false));      // (rows of the host part alone)
    run(dk ? "one path, need_dk" : "one path", sizes(22, 1, 1, 0, 0, 0, 0, 0, dk, false));
  }
  run("claim without a batch", sizes(8191, 0, 0, 0, 0, 0, 0, 0, false, true));
  run("claim with a batch", sizes(50000, 640, 1900, 33, 71, 150, 4001, 333, false, true));
  run("claim, a batch without alleles and rows", sizes(300, 2, 0, 1, 0, 0, 0, 0, false, true));
  run("claim, tables but no cluster", sizes(300, 0, 0, 0, 5, 9, 64, 64, false, true));
  printf("%s (%d mismatches, %d cases)\n", bad ? "FAILED" : "OK", bad, cases);
  return bad ? 1 : 0;
}
