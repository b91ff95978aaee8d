// mfx_bin.h -- the plain arithmetic of -bin (include/merfin_amd.h: mfx_bin_*; the driver: mfx_bin.cpp; the kernel: mfx_kernels.hip,
// mfx_bin_kernel): how records are cut into batches, which PIECES of records a batch holds, how the pieces' counts are folded into the
// records, and the class rule.  One text for the device path (mfx_bin.cpp, mfx_reads.cpp), for mfx_bin_plan_host / mfx_bin_classify and
// for tools/native/bin_sanitize.cpp.  No HIP call, no library state: g++ compiles it alone.
//
// THE CUT (what mfx_reads_add, mfx_reads_store_add and mfx_bin_add share: mfx_batch_records).  Records are copied back to back into a byte
// batch, one 'N' between two; a record longer than the room left is cut, and its rest starts the next batch k-1 bases before the cut, so
// every k-mer of a record lies in exactly one batch.  A PIECE is the part of one record inside one batch: pieces of a batch ascend with
// their first position, two of them are separated by the 'N', and none is shorter than k (a batch with less than k bases of room goes
// before the record is cut into it, and the rest of a cut record holds at least k bases).
//
// THE CLASS RULE is this project's own, in the spirit of Canu's haplotype split (TrioCanu); it is not validated against Canu.  With
// NA = norm_a ? norm_a : 1 and NB likewise (the sizes of the two hap-mer sets), a read of `a` A-only and `b` B-only k-mers is
//   A        iff  a + b >= min_hits  and  a * NB * 1000 > b * NA * ratio_milli
//   B        iff  a + b >= min_hits  and  b * NA * 1000 > a * NB * ratio_milli
//   unknown  otherwise (ties, a = b = 0),
// the products in 128 bits (2^32 * 4^31 * 2^32 fits).  ratio_milli >= 1000: below that both conditions could hold.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

constexpr uint64_t MFX_BATCH_BASES_DEFAULT = 1ull << 26;     // bases per batch: 24 MB of planes per stage
constexpr uint64_t MFX_BATCH_BASES_MAX = 1ull << 34;
constexpr uint64_t MFX_BIN_TILE = 4096;                      // MFX_TILE (mfx_internal.h), restated: this header includes nothing of the library

inline uint64_t mfx_batch_bases_min(int k) { return 2ull * (uint64_t)k + 2; }

// The bytes of the batch being filled.  `bytes` empty: nothing is copied (the plan alone: mfx_bin_plan_host).
struct mfx_batch {
  uint64_t cap = 0;                  // bases per batch
  std::vector<uint8_t> bytes;
  uint64_t used = 0;
};

// Records into batches.  Whenever a batch is complete `flush` is called (it sends or keeps b.bytes[0, b.used) and sets b.used = 0;
// non-zero: its error, passed on).  piece(i, first, len, last): record i of this call has bases [first, first + len) of the batch being
// filled; last: they end the record.  no_bases(i): record i holds k-mers and has no text; its result is returned.  bases == nullptr:
// lengths only (nothing is copied, no_bases is not asked).
template <class NoBases, class Flush, class Piece>
int mfx_batch_records(mfx_batch &b, uint64_t k, const char *const *bases, const uint64_t *lens, uint64_t n, uint64_t &n_reads, uint64_t &n_bases,
                      NoBases &&no_bases, Flush &&flush, Piece &&piece) {
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t len = lens[i];
    n_reads += 1;
    n_bases += len;
    if (len < k) continue;                                     // no k-mer
    if (bases && !bases[i]) return no_bases(i);
    const uint8_t *src = bases ? reinterpret_cast<const uint8_t *>(bases[i]) : nullptr;
    uint64_t at = 0;
    while (true) {
      if (b.cap - b.used < k) {                                // no whole k-mer fits: the batch goes
        if (int rc = flush()) return rc;
      }
      const uint64_t take = std::min(len - at, b.cap - b.used);
      if (src) memcpy(b.bytes.data() + b.used, src + at, take);
      piece(i, b.used, take, at + take == len);
      b.used += take;
      if (at + take == len) {
        if (b.used < b.cap) {                                  // (a read that ends the batch needs no separator)
          if (src) b.bytes[b.used] = 'N';
          b.used++;
        }
        break;
      }
      at += take - (k - 1);                                    // the rest, from the first k-mer this batch does not hold
      if (int rc = flush()) return rc;
    }
  }
  return 0;
}

// ---- the piece plan -----------------------------------------------------------------------------------------------------------------
struct mfx_bin_piece {
  uint64_t record;                   // the number of its record (the caller's numbering)
  uint64_t first, len;               // bases [first, first + len) of the batch
  bool     last;                     // the record ends with this piece
};

// per tile of a batch of npos positions: the first piece that touches the tile -- the first whose last base lies at or behind the tile's
// first position (n: none does).  The pieces ascend, so a tile's pieces are tile_first[t], tile_first[t] + 1, ... while they start in it.
inline void mfx_bin_tile_first(const mfx_bin_piece *p, uint64_t n, uint64_t npos, uint64_t *tile_first) {
  const uint64_t ntiles = (npos + MFX_BIN_TILE - 1) / MFX_BIN_TILE;
  uint64_t q = 0;
  for (uint64_t t = 0; t < ntiles; ++t) {
    while (q < n && p[q].first + p[q].len <= t * MFX_BIN_TILE) ++q;
    tile_first[t] = q;
  }
}

// the k-mers of a piece of len bases
inline uint64_t mfx_bin_piece_kmers(uint64_t len, uint64_t k) { return len >= k ? len - k + 1 : 0; }

// ---- the fold -----------------------------------------------------------------------------------------------------------------------
// counts[i][4] (k-mers, A only, B only, shared) of piece i are added to its record; rec(record) gives the record's four uint32.  In piece
// order, which is input order; a record's totals stay below 2^32 (it has fewer than 2^32 bases).
template <class Rec>
void mfx_bin_fold(const mfx_bin_piece *p, uint64_t n, const uint32_t *counts, Rec &&rec) {
  for (uint64_t i = 0; i < n; ++i) {
    uint32_t *r = rec(p[i].record);
    for (int f = 0; f < 4; ++f) r[f] += counts[4 * i + f];
  }
}

// ---- the class rule -----------------------------------------------------------------------------------------------------------------
enum { MFX_BIN_A = 0, MFX_BIN_B = 1, MFX_BIN_UNKNOWN = 2 };

inline int mfx_bin_class(uint32_t a, uint32_t b, uint64_t norm_a, uint64_t norm_b, uint32_t ratio_milli, uint32_t min_hits) {
  typedef unsigned __int128 u128;
  const u128 NA = norm_a ? norm_a : 1, NB = norm_b ? norm_b : 1;
  if ((uint64_t)a + (uint64_t)b < (uint64_t)min_hits) return MFX_BIN_UNKNOWN;
  const u128 wa = (u128)a * NB, wb = (u128)b * NA;             // a / NA against b / NB, cross-multiplied
  if (wa * 1000u > wb * ratio_milli) return MFX_BIN_A;
  if (wb * 1000u > wa * ratio_milli) return MFX_BIN_B;
  return MFX_BIN_UNKNOWN;
}
