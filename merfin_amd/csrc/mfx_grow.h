// mfx_grow.h -- the plain host arithmetic of the claiming read counter's table (mfx_reads.cpp) and of mfx_index_write_db's key ranges
// (mfx_db.cpp), and the key ranges of the passes of `merfin -count -passes` (mfx_cut_bins).  No HIP, no library state:
// tools/native/grow_sanitize.cpp and tools/native/cuts_sanitize.cpp drive it under the sanitizers.
#pragma once
#include <stdint.h>

#include <vector>

// ---- a table that grows ----------------------------------------------------------------------------------------------------------
// A launch never overfills the table: a batch of B positions is enqueued only while
//   distinct + pending + B <= 0.7 x slots          (0.7: the smallest load factor of a full table, MFX_LF_MAX)
// holds, where `distinct` is the table's meta[0] as last read and `pending` the positions enqueued since that read (each of them may
// claim one k-mer).  All in integers: 10 (d + p + B) <= 7 slots.
inline bool mfx_grow_fits(uint64_t distinct, uint64_t pending, uint64_t B, uint64_t slots) {
  const unsigned __int128 need = (unsigned __int128)distinct + pending + B;
  return need * 10u <= (unsigned __int128)slots * 7u;
}

// The table a counter grows into: the smallest power-of-two multiple (>= 2) of the current lines for which
//   distinct + B <= 0.35 x slots                   (20 (d + B) <= 7 slots)
// so that a grown table takes at least as many claims again as it holds before it has to grow once more.  0: no such table below
// max_lines (the device numbers its lines in 32 bits).
inline uint64_t mfx_grow_lines(uint64_t distinct, uint64_t B, uint64_t nlines, uint32_t slots_line, uint64_t max_lines) {
  if (nlines == 0 || slots_line == 0) return 0;
  const unsigned __int128 need = ((unsigned __int128)distinct + B) * 20u;
  for (uint64_t mult = 2; mult != 0 && nlines <= max_lines / mult; mult <<= 1) {
    const uint64_t nl = nlines * mult;
    if (need <= (unsigned __int128)nl * slots_line * 7u) return nl;
  }
  return 0;
}

// ---- key ranges of a sorted export ---------------------------------------------------------------------------------------------------
// bins[b]: entries whose top key bits are b.  Consecutive bins are grouped into ranges [bin_lo, bin_hi) of at most R entries each; a
// bin that alone holds more than R is a range of its own (the caller sizes its buffers by the largest range).  Empty bins join the range
// before them or are skipped: no range is empty, the ranges are ascending and together hold every non-empty bin.
struct mfx_bin_range { uint32_t bin_lo, bin_hi; uint64_t n; };

inline void mfx_group_bins(const uint64_t *bins, uint32_t nbins, uint64_t R, std::vector<mfx_bin_range> &out) {
  out.clear();
  if (R == 0) R = 1;
  mfx_bin_range cur{0, 0, 0};
  for (uint32_t b = 0; b < nbins; ++b) {
    const uint64_t c = bins[b];
    if (c == 0) continue;
    if (cur.n != 0 && (c > R || cur.n > R - c)) {             // (cur.n + c > R without the overflow)
      out.push_back(cur);
      cur.n = 0;
    }
    if (cur.n == 0) cur.bin_lo = b;
    cur.bin_hi = b + 1;
    cur.n += c;
  }
  if (cur.n != 0) out.push_back(cur);
}

// ---- key ranges of the passes of a count ---------------------------------------------------------------------------------------------
// The bins [bin_lo, bin_hi) cut at bin boundaries into consecutive ranges that together are [bin_lo, bin_hi) -- a bin without entries here
// may hold some in a later pass, so it belongs to a range too.  No range lacks entries, so there are min(parts, non-empty bins) ranges
// (none when no bin holds an entry).  The cuts are chosen so that the largest range's mass is minimal; of the cuttings that reach it the
// first in ascending order of the cuts wins (every cut as early as the others still allow).  Masses are summed in 128 bits; a range's n
// saturates at 2^64 - 1.
inline void mfx_cut_bins(const uint64_t *bins, uint32_t bin_lo, uint32_t bin_hi, uint32_t parts, std::vector<mfx_bin_range> &out) {
  typedef unsigned __int128 u128;
  out.clear();
  if (bin_hi <= bin_lo || parts == 0) return;
  const uint32_t nb = bin_hi - bin_lo;
  const uint64_t *b = bins + bin_lo;
  u128 total = 0;
  uint64_t largest = 0;
  uint32_t nonempty = 0;
  for (uint32_t i = 0; i < nb; ++i) {
    total += b[i];
    if (b[i] > largest) largest = b[i];
    if (b[i]) ++nonempty;
  }
  if (nonempty == 0) return;
  const uint32_t m = parts < nonempty ? parts : nonempty;
  // need[c]: the fewest ranges of mass <= T that hold the bins from c on (0 at the end); nxt: where the longest such range from c ends
  std::vector<uint32_t> need(nb + 1), ne(nb + 1);
  auto fewest = [&](u128 T) {
    need[nb] = 0;
    u128 sum = 0;
    uint32_t e = nb;                                           // the range from c ends at e: [c, e) has mass `sum` <= T, and is as long as T allows
    for (uint32_t c = nb; c-- > 0;) {
      sum += b[c];
      while (sum > T) sum -= b[--e];
      need[c] = 1 + need[e];
    }
    return need[0];
  };
  u128 lo = largest, hi = total;                               // the smallest T with fewest(T) <= m
  while (lo < hi) {
    const u128 mid = lo + (hi - lo) / 2;
    if (fewest(mid) <= m) hi = mid; else lo = mid + 1;
  }
  const u128 T = lo;
  fewest(T);
  ne[nb] = 0;
  for (uint32_t c = nb; c-- > 0;) ne[c] = ne[c + 1] + (b[c] ? 1u : 0u);
  uint32_t at = 0;
  for (uint32_t left = m; left > 0; --left) {
    mfx_bin_range r{bin_lo + at, bin_hi, 0};
    u128 sum = 0;
    uint32_t c = at;
    if (left == 1) {
      for (; c < nb; ++c) sum += b[c];
    } else {
      // the earliest end c: the range holds entries, and the bins from c on make exactly left - 1 ranges
      while (true) {
        sum += b[c++];
        if (sum != 0 && need[c] <= left - 1 && left - 1 <= ne[c]) break;
      }
    }
    r.bin_hi = bin_lo + c;
    r.n = sum > (u128)~0ull ? ~0ull : (uint64_t)sum;
    out.push_back(r);
    at = c;
  }
}
