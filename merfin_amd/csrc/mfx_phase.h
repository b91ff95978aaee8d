// mfx_phase.h -- the shared text of -phase (include/merfin_amd.h: mfx_phase_run): hap-mer markers of two parents -> runs of one
// haplotype -> phase blocks with their switch errors.  Three layers include it:
//   - the evaluation kernels (mfx_kernels.hip: mfx_phase_mark_kernel; mfx_wide.hip: its 128-bit twin) take the two ballots and the
//     per-contig totals from the device part below;
//   - the plane kernels (mfx_phase.hip) and the host restatement (mfx_phase_planes_host below, exported as mfx_phase_from_planes_host;
//     tools/native/phase_sanitize.cpp drives it under the sanitizers) run ONE text for the word arithmetic: the carried marker, the
//     operator that joins two carries, where a run starts inside a word, when a run is long, when it opens a block, a block's haplotype;
//   - the driver (mfx_phase.cpp) sizes the arrays after the counts and writes the three texts.
//
// THE PLANES are laid out as -regions' (csrc/mfx_regions.h): [2][ntiles * 64], bit b of plane[h][tile * 64 + w] is position 64 w + b of the
// tile; plane 0: the k-mer is in A and not in B, plane 1: in B and not in A; no position is in both; words beyond a contig's end are 0.
//
// THE RULE (sequential; tests/phase_ref.py walks it literally).  The markers of a contig are its flagged positions in ascending order.  A
// run is a maximal stretch of consecutive markers of one haplotype (unflagged positions between them are transparent), n markers,
// span = last - first + k bases; it is short iff n <= S and span <= R, else long.  A block opens at a contig's first run and at every long
// run whose nearest earlier long run of the contig has the other haplotype; every other run joins the open block.  A block's haplotype is
// that of its long runs; a block without one (the only block of a contig without one) takes the haplotype with more markers, a tie 0.
//
// ON THE DEVICE this is one associative operator used twice -- "the last non-empty value, reset at a contig's first element"
// (mfx_ph_join): over the words / tiles it carries the last marker (position and haplotype) in front of a word, which says where a run
// starts and where the run in front of it ended; over the run list it carries the haplotype of the nearest earlier long run, which says
// where a block opens.  A popcount scan ranks the markers, so a run's n is a difference of ranks; a block's sums are differences of
// exclusive scans of the runs' A and B counts.
#pragma once
#include <stdint.h>
#include <vector>

#include "../../include/merfin_amd.h"
#include "mfx_regions.h"                                      // the tile, the position of a bit, mfx_rg_pop_bit

constexpr uint32_t MFX_PH_REC_WORDS = 6;                      // mfx_phase_block as the kernels address it
constexpr uint64_t MFX_PH_RESET = 1ull << 63;                 // on a carry: the element is its contig's first

// ---- the carried value: a marker (0: none), or for the run list a haplotype + 1 (0: none) -------------------------------------
MFX_HD uint64_t mfx_ph_mark(uint64_t pos, uint32_t hap) { return ((pos << 1) | (uint64_t)hap) + 1ull; }
MFX_HD uint32_t mfx_ph_mark_hap(uint64_t v) { return (uint32_t)((v - 1ull) & 1ull); }
MFX_HD uint64_t mfx_ph_mark_pos(uint64_t v) { return (v - 1ull) >> 1; }
MFX_HD uint64_t mfx_ph_value(uint64_t e) { return e & ~MFX_PH_RESET; }

// a then b: the last non-empty value, nothing of a beyond an element that is its contig's first
MFX_HD uint64_t mfx_ph_join(uint64_t a, uint64_t b) {
  if (b & MFX_PH_RESET) return b;
  return mfx_ph_value(b) ? ((a & MFX_PH_RESET) | b) : a;
}

// ---- the word arithmetic: m = plane 0 | plane 1 (the markers), h = plane 1 (their haplotypes) ------------------------------------
// the last marker of a word whose bit 0 is position pos0
MFX_HD uint64_t mfx_ph_word_last(uint64_t m, uint64_t h, uint64_t pos0) {
  if (!m) return 0ull;
  const uint32_t b = 63u - (uint32_t)__builtin_clzll(m);
  return mfx_ph_mark(pos0 + b, (uint32_t)((h >> b) & 1ull));
}
// the markers of a word that start a run; prev: the marker in front of the word (0: none in this contig)
MFX_HD uint64_t mfx_ph_starts(uint64_t m, uint64_t h, uint64_t prev) {
  uint64_t s = 0ull;
  uint32_t before = prev ? 1u + mfx_ph_mark_hap(prev) : 0u;
  while (m) {
    const uint32_t b = mfx_rg_pop_bit(m);
    const uint32_t cur = 1u + (uint32_t)((h >> b) & 1ull);
    if (cur != before) s |= 1ull << b;
    before = cur;
  }
  return s;
}
// markers of the word below bit b; the marker in front of bit b (prev: the one in front of the word)
MFX_HD uint32_t mfx_ph_below(uint64_t m, uint32_t b) { return (uint32_t)__builtin_popcountll(m & ((1ull << b) - 1ull)); }
MFX_HD uint64_t mfx_ph_before(uint64_t m, uint64_t h, uint32_t b, uint64_t pos0, uint64_t prev) {
  const uint64_t lo = m & ((1ull << b) - 1ull);
  return lo ? mfx_ph_word_last(lo, h, pos0) : prev;
}

// ---- the run and block rules --------------------------------------------------------------------------------------------------
// a run of n markers, first at `start`, `end` = its last marker + 1
MFX_HD bool mfx_ph_long(uint64_t n, uint64_t start, uint64_t end, uint64_t k, uint64_t S, uint64_t R) {
  return !(n <= S && end - 1ull - start + k <= R);
}
// prev_long: haplotype + 1 of the nearest earlier long run of the contig (0: none)
MFX_HD bool mfx_ph_head(bool contig_first, bool is_long, uint32_t hap, uint64_t prev_long) {
  return contig_first || (is_long && prev_long != 0ull && prev_long != (uint64_t)hap + 1ull);
}
// last_long: haplotype + 1 of the last long run at or before the block's last run (0: the block has none)
MFX_HD uint32_t mfx_ph_block_hap(uint64_t last_long, uint64_t nA, uint64_t nB) {
  return last_long ? (uint32_t)(last_long - 1ull) : (nB > nA ? 1u : 0u);
}
// runs of a contig alternate: of the nruns runs of a block whose first has haplotype first_hap, those of the other haplotype than `hap`
MFX_HD uint64_t mfx_ph_other_runs(uint64_t nruns, uint32_t first_hap, uint32_t hap) {
  return first_hap == hap ? nruns / 2ull : (nruns + 1ull) / 2ull;
}

// ---- the same steps on the host -----------------------------------------------------------------------------------------------
// planes -> records, step by step as the device takes them.  planes: [2][ntiles * 64]; tile_start: [ncontigs + 1]; tile_contig: [ntiles].
inline void mfx_phase_planes_host(const uint64_t *planes, uint64_t ntiles, const uint64_t *tile_start, const uint32_t *tile_contig, uint64_t k,
                                  uint64_t S, uint64_t R, std::vector<mfx_phase_block> &out) {
  out.clear();
  const uint64_t nw = ntiles * MFX_RG_WORDS;
  const uint64_t *p0 = planes, *p1 = planes + nw;
  auto first_tile = [&](uint64_t t) { return t == 0 || tile_contig[t - 1] != tile_contig[t]; };
  auto last_tile = [&](uint64_t t) { return t + 1 == ntiles || tile_contig[t + 1] != tile_contig[t]; };
  // the tile kernel: a tile's markers and its last marker; then the two scans
  std::vector<uint64_t> rank0((size_t)ntiles + 1, 0), car((size_t)ntiles, 0);
  for (uint64_t t = 0; t < ntiles; ++t) {
    uint64_t n = 0, last = 0;
    for (uint64_t i = t * MFX_RG_WORDS; i < (t + 1) * MFX_RG_WORDS; ++i) {
      const uint64_t m = p0[i] | p1[i];
      n += (uint64_t)__builtin_popcountll(m);
      last = mfx_ph_join(last, mfx_ph_word_last(m, p1[i], mfx_rg_position(tile_start, tile_contig[t], i, 0)));
    }
    rank0[t] = n;
    car[t] = (first_tile(t) ? MFX_PH_RESET : 0ull) | last;
  }
  uint64_t sum = 0;
  for (uint64_t t = 0; t <= ntiles; ++t) { const uint64_t n = rank0[t]; rank0[t] = sum; sum += n; }
  for (uint64_t t = 1; t < ntiles; ++t) car[t] = mfx_ph_join(car[t - 1], car[t]);
  const uint64_t nmarkers = rank0[ntiles];
  auto tile_in = [&](uint64_t t) { return first_tile(t) ? 0ull : mfx_ph_value(car[t - 1]); };
  // the count kernel, its scan
  std::vector<uint64_t> off((size_t)ntiles + 1, 0);
  for (uint64_t t = 0; t < ntiles; ++t) {
    uint64_t prev = tile_in(t), n = 0;
    for (uint64_t i = t * MFX_RG_WORDS; i < (t + 1) * MFX_RG_WORDS; ++i) {
      const uint64_t m = p0[i] | p1[i];
      n += (uint64_t)__builtin_popcountll(mfx_ph_starts(m, p1[i], prev));
      prev = mfx_ph_join(prev, mfx_ph_word_last(m, p1[i], mfx_rg_position(tile_start, tile_contig[t], i, 0)));
    }
    off[t] = n;
  }
  sum = 0;
  for (uint64_t t = 0; t <= ntiles; ++t) { const uint64_t n = off[t]; off[t] = sum; sum += n; }
  const uint64_t nruns = off[ntiles];
  if (nruns == 0) return;
  // the scatter kernel: a run's contig, haplotype, first marker and that marker's rank; the marker in front of it ends the run in front
  // of it; a contig's last marker ends the last run listed up to the contig's last tile
  std::vector<uint32_t> rc((size_t)nruns), rh((size_t)nruns);
  std::vector<uint64_t> rs((size_t)nruns), re((size_t)nruns), rr((size_t)nruns);
  for (uint64_t t = 0; t < ntiles; ++t) {
    const uint32_t c = tile_contig[t];
    uint64_t prev = tile_in(t), at = off[t], rank = rank0[t];
    for (uint64_t i = t * MFX_RG_WORDS; i < (t + 1) * MFX_RG_WORDS; ++i) {
      const uint64_t m = p0[i] | p1[i];
      uint64_t s = mfx_ph_starts(m, p1[i], prev);
      while (s) {
        const uint32_t b = mfx_rg_pop_bit(s);
        rc[at] = c;
        rh[at] = (uint32_t)((p1[i] >> b) & 1ull);
        rs[at] = mfx_rg_position(tile_start, c, i, b);
        rr[at] = rank + mfx_ph_below(m, b);
        const uint64_t before = mfx_ph_before(m, p1[i], b, mfx_rg_position(tile_start, c, i, 0), prev);
        if (before) re[at - 1] = mfx_ph_mark_pos(before) + 1ull;
        ++at;
      }
      rank += (uint64_t)__builtin_popcountll(m);
      prev = mfx_ph_join(prev, mfx_ph_word_last(m, p1[i], mfx_rg_position(tile_start, c, i, 0)));
    }
    if (last_tile(t) && mfx_ph_value(car[t])) re[off[t + 1] - 1] = mfx_ph_mark_pos(mfx_ph_value(car[t])) + 1ull;
  }
  // the runs kernel: long or short, the carried haplotype of long runs, the A and B markers; the three scans
  std::vector<uint64_t> lng((size_t)nruns), ax((size_t)nruns + 1, 0), bx((size_t)nruns + 1, 0), head((size_t)nruns + 1, 0);
  auto first_run = [&](uint64_t i) { return i == 0 || rc[i - 1] != rc[i]; };
  for (uint64_t i = 0; i < nruns; ++i) {
    const uint64_t n = (i + 1 < nruns ? rr[i + 1] : nmarkers) - rr[i];
    const bool is_long = mfx_ph_long(n, rs[i], re[i], k, S, R);
    lng[i] = (first_run(i) ? MFX_PH_RESET : 0ull) | (is_long ? (uint64_t)rh[i] + 1ull : 0ull);
    ax[i] = rh[i] == 0 ? n : 0;
    bx[i] = rh[i] == 1 ? n : 0;
  }
  std::vector<uint64_t> own(lng);                             // (the device keeps the elements: a run's own value is read again)
  for (uint64_t i = 1; i < nruns; ++i) lng[i] = mfx_ph_join(lng[i - 1], lng[i]);
  uint64_t sa = 0, sb = 0;
  for (uint64_t i = 0; i <= nruns; ++i) { const uint64_t a = ax[i], b = bx[i]; ax[i] = sa; bx[i] = sb; sa += a; sb += b; }
  // the heads kernel, its scan, the bounds, the records
  for (uint64_t i = 0; i < nruns; ++i)
    head[i] = mfx_ph_head(first_run(i), mfx_ph_value(own[i]) != 0, rh[i], first_run(i) ? 0ull : mfx_ph_value(lng[i - 1])) ? 1ull : 0ull;
  sum = 0;
  for (uint64_t i = 0; i <= nruns; ++i) { const uint64_t n = head[i]; head[i] = sum; sum += n; }
  const uint64_t nblocks = head[nruns];
  std::vector<uint64_t> bf((size_t)nblocks), bl((size_t)nblocks);
  for (uint64_t i = 0; i < nruns; ++i) {
    const uint64_t r = head[i + 1] - 1ull;
    if (head[i + 1] != head[i]) bf[r] = i;
    if (i + 1 == nruns || head[i + 2] != head[i + 1]) bl[r] = i;
  }
  out.resize((size_t)nblocks);
  for (uint64_t r = 0; r < nblocks; ++r) {
    const uint64_t f = bf[r], l = bl[r];
    const uint64_t nA = ax[l + 1] - ax[f], nB = bx[l + 1] - bx[f];
    const uint32_t hap = mfx_ph_block_hap(mfx_ph_value(lng[l]), nA, nB);
    mfx_phase_block &x = out[r];
    x.contig = rc[f];
    x.hap = hap;
    x.start = rs[f];
    x.end = re[l];
    x.n_hap = hap ? nB : nA;
    x.n_switch = hap ? nA : nB;
    x.n_switch_runs = mfx_ph_other_runs(l - f + 1ull, rh[f], hap);
  }
}

// ---- device part: the two ballots of a wave's 64 positions, the totals of a tile ------------------------------------------------
#if defined(MFX_PHASE_DEVICE)                                 // the kernel files define it in front of this header
struct mfx_ph_acc { uint32_t valid, a, b, shared; };          // wave-uniform: what this wave met of the tile

// ok: a valid k-mer; rv / av: its values on the read side (A) and the assembly side (B).  One lane stores the two words: plain vector stores.
__device__ __forceinline__ void mfx_ph_store_masks(uint64_t *planes, uint64_t nwords, uint64_t word, bool ok, uint32_t rv, uint32_t av, mfx_ph_acc &acc) {
  const bool inA = ok && rv != 0u, inB = ok && av != 0u;
  const uint64_t mv = __ballot(ok), ma = __ballot(inA && !inB), mb = __ballot(inB && !inA), ms = __ballot(inA && inB);
  acc.valid += (uint32_t)__popcll(mv);
  acc.a += (uint32_t)__popcll(ma);
  acc.b += (uint32_t)__popcll(mb);
  acc.shared += (uint32_t)__popcll(ms);
  if ((threadIdx.x & 63u) == 0u) {
    planes[word] = ma;
    planes[nwords + word] = mb;
  }
}
// a wave's totals of one tile to its contig's four counts: integer sums, the same in any order
__device__ __forceinline__ void mfx_ph_add_counts(uint64_t *counts, uint32_t contig, const mfx_ph_acc &acc) {
  if ((threadIdx.x & 63u) != 0u) return;
  unsigned long long *c = reinterpret_cast<unsigned long long *>(counts + 4ull * contig);
  if (acc.valid) (void)__hip_atomic_fetch_add(c + 0, (unsigned long long)acc.valid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (acc.a) (void)__hip_atomic_fetch_add(c + 1, (unsigned long long)acc.a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (acc.b) (void)__hip_atomic_fetch_add(c + 2, (unsigned long long)acc.b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (acc.shared) (void)__hip_atomic_fetch_add(c + 3, (unsigned long long)acc.shared, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
#endif
