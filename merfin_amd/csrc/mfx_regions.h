// mfx_regions.h -- the shared text of -regions (include/merfin_amd.h: mfx_regions_run): maximal runs of missing, collapsed and
// expanded k-mers as intervals.  Three layers include it:
//   - the evaluation kernels (mfx_kernels.hip: mfx_regions_class_kernel / mfx_regions_sums_kernel; mfx_wide.hip: their 128-bit twins)
//     take the class rule, the wave's share of a region and the search of a position's region from the device part below;
//   - the plane kernels (mfx_regions.hip) and the host restatement (mfx_regions_planes_host below, exported as
//     mfx_regions_from_planes_host; tools/native/regions_sanitize.cpp drives it under the sanitizers) run ONE text for the word
//     arithmetic: where runs start and end inside a 64-bit word of a class plane, which neighbour bit counts, and when a run opens
//     a new region;
//   - the driver (mfx_regions.cpp) orders the three classes' lists into the records' order.
//
// THE PLANES.  A tile is MFX_TILE = 4096 start positions of one contig; in a round of a tile's evaluation lane `tid` holds position
// round * 256 + tid, so wave w of round r holds the 64 consecutive positions of word r * 4 + w: bit b of plane[cls][tile * 64 + word] is
// position word * 64 + b of the tile.  A contig's tiles are consecutive, so its words are; positions beyond a contig's end are 0.
// A run therefore continues from bit 63 of a word into bit 0 of the next word of the SAME contig, and into nothing else.
#pragma once
#include <stdint.h>
#include <vector>

#include "../../include/merfin_amd.h"
#include "mfx_kstar.h"

constexpr uint32_t MFX_RG_CLASSES = 3;                       // MFX_REGION_MISSING, _COLLAPSED, _EXPANDED
constexpr uint32_t MFX_RG_NONE = 3;                          // a position in no class
constexpr uint32_t MFX_RG_TILE = 4096;                       // == MFX_TILE (mfx_internal.h; the kernel files assert it)
constexpr uint32_t MFX_RG_WORDS = MFX_RG_TILE / 64;          // words per tile and class
constexpr uint32_t MFX_RG_REC_WORDS = 7;                     // mfx_region as the kernels address it

// ---- the word arithmetic (host and device) ----------------------------------------------------------------------------------
// bits of w where a run starts / ends (its last flagged position), given the bit in front of bit 0 / behind bit 63
MFX_HD uint64_t mfx_rg_starts(uint64_t w, uint64_t prev_msb) { return w & ~((w << 1) | prev_msb); }
MFX_HD uint64_t mfx_rg_ends(uint64_t w, uint64_t next_lsb) { return w & ~((w >> 1) | (next_lsb << 63)); }

// the neighbour bits of word i of a class plane of nwords words: the adjacent word counts when it lies in a tile of the same contig
MFX_HD uint64_t mfx_rg_prev_msb(const uint64_t *plane, const uint32_t *tile_contig, uint64_t i) {
  if (i == 0) return 0;
  if (tile_contig[(i - 1) / MFX_RG_WORDS] != tile_contig[i / MFX_RG_WORDS]) return 0;
  return plane[i - 1] >> 63;
}
MFX_HD uint64_t mfx_rg_next_lsb(const uint64_t *plane, const uint32_t *tile_contig, uint64_t nwords, uint64_t i) {
  if (i + 1 >= nwords) return 0;
  if (tile_contig[(i + 1) / MFX_RG_WORDS] != tile_contig[i / MFX_RG_WORDS]) return 0;
  return plane[i + 1] & 1ull;
}

// start position (inside its contig) of bit b of word i
MFX_HD uint64_t mfx_rg_position(const uint64_t *tile_start, uint32_t contig, uint64_t i, uint32_t b) {
  return (i / MFX_RG_WORDS - tile_start[contig]) * MFX_RG_TILE + (i % MFX_RG_WORDS) * 64 + b;
}

// Does run i open a region?  The runs of one class lie in (contig, start) order; `first`: no run of the class precedes it.  end is
// exclusive, so start - prev_end is the number of positions between the two runs.
MFX_HD bool mfx_rg_head(bool first, uint32_t prev_contig, uint64_t prev_end, uint32_t contig, uint64_t start, uint64_t gap) {
  return first || prev_contig != contig || start - prev_end > gap;
}

// lowest set bit's number, cleared from w
MFX_HD uint32_t mfx_rg_pop_bit(uint64_t &w) {
  const uint32_t b = (uint32_t)__builtin_ctzll(w);
  w &= w - 1;
  return b;
}

// ---- the same steps on the host ---------------------------------------------------------------------------------------------
// (a)  (class, contig, start) order -> the records' order: contig, start, class.  cls_begin[c] .. cls_begin[c + 1]: class c's records.
inline void mfx_rg_order(const mfx_region *in, const uint64_t *cls_begin, std::vector<mfx_region> &out) {
  uint64_t at[MFX_RG_CLASSES];
  for (uint32_t c = 0; c < MFX_RG_CLASSES; ++c) at[c] = cls_begin[c];
  out.clear();
  out.reserve((size_t)(cls_begin[MFX_RG_CLASSES] - cls_begin[0]));
  for (;;) {
    int best = -1;
    for (uint32_t c = 0; c < MFX_RG_CLASSES; ++c) {
      if (at[c] == cls_begin[c + 1]) continue;
      const mfx_region &x = in[at[c]];
      if (best < 0 || x.contig < in[at[best]].contig || (x.contig == in[at[best]].contig && x.start < in[at[best]].start)) best = (int)c;
    }
    if (best < 0) break;
    out.push_back(in[at[best]++]);
  }
}

// (b)  planes -> records, step by step as the device takes them: counts per (class, tile), their exclusive scan, the scatter of starts and
// ends, the heads, their scan, the regions, the filter.  planes: [3][ntiles * 64]; tile_start: [ncontigs + 1]; tile_contig: [ntiles].
// The sums and ext_kstar of a record are pass 2's and stay 0 here.
inline void mfx_regions_planes_host(const uint64_t *planes, uint64_t ntiles, const uint64_t *tile_start, const uint32_t *tile_contig,
                                    uint64_t gap, uint64_t min_kmers, std::vector<mfx_region> &out) {
  const uint64_t nw = ntiles * MFX_RG_WORDS, nct = ntiles * MFX_RG_CLASSES;
  std::vector<uint64_t> off_s(nct + 1, 0), off_e(nct + 1, 0);
  for (uint64_t ct = 0; ct < nct; ++ct) {                     // the count kernel: one wave per (class, tile)
    const uint64_t *plane = planes + (ct / ntiles) * nw;
    uint64_t ns = 0, ne = 0;
    for (uint64_t i = (ct % ntiles) * MFX_RG_WORDS; i < (ct % ntiles + 1) * MFX_RG_WORDS; ++i) {
      ns += (uint64_t)__builtin_popcountll(mfx_rg_starts(plane[i], mfx_rg_prev_msb(plane, tile_contig, i)));
      ne += (uint64_t)__builtin_popcountll(mfx_rg_ends(plane[i], mfx_rg_next_lsb(plane, tile_contig, nw, i)));
    }
    off_s[ct] = ns;
    off_e[ct] = ne;
  }
  uint64_t run_s = 0, run_e = 0;
  for (uint64_t ct = 0; ct <= nct; ++ct) {                    // the exclusive scans
    const uint64_t s = off_s[ct], e = off_e[ct];
    off_s[ct] = run_s; off_e[ct] = run_e;
    run_s += s; run_e += e;
  }
  const uint64_t nruns = off_s[nct];
  std::vector<uint32_t> rc((size_t)nruns);
  std::vector<uint64_t> rs((size_t)nruns), re((size_t)nruns);
  for (uint64_t ct = 0; ct < nct; ++ct) {                     // the scatter kernel
    const uint64_t *plane = planes + (ct / ntiles) * nw;
    const uint32_t c = tile_contig[ct % ntiles];
    uint64_t is = off_s[ct], ie = off_e[ct];
    for (uint64_t i = (ct % ntiles) * MFX_RG_WORDS; i < (ct % ntiles + 1) * MFX_RG_WORDS; ++i) {
      uint64_t s = mfx_rg_starts(plane[i], mfx_rg_prev_msb(plane, tile_contig, i));
      uint64_t e = mfx_rg_ends(plane[i], mfx_rg_next_lsb(plane, tile_contig, nw, i));
      while (s) { rc[is] = c; rs[is++] = mfx_rg_position(tile_start, c, i, mfx_rg_pop_bit(s)); }
      while (e) re[ie++] = mfx_rg_position(tile_start, c, i, mfx_rg_pop_bit(e)) + 1;
    }
  }
  uint64_t cls_run[MFX_RG_CLASSES + 1];
  for (uint32_t c = 0; c <= MFX_RG_CLASSES; ++c) cls_run[c] = off_s[c * ntiles];
  std::vector<mfx_region> raw;
  uint64_t cls_reg[MFX_RG_CLASSES + 1] = {0, 0, 0, 0};
  for (uint32_t cls = 0; cls < MFX_RG_CLASSES; ++cls) {       // heads, regions, filter
    std::vector<mfx_region> mine;
    for (uint64_t i = cls_run[cls]; i < cls_run[cls + 1]; ++i) {
      const bool first = i == cls_run[cls];
      if (mfx_rg_head(first, first ? 0u : rc[i - 1], first ? 0ull : re[i - 1], rc[i], rs[i], gap)) {
        mfx_region r;
        r.contig = rc[i]; r.cls = cls; r.start = rs[i]; r.end = re[i]; r.n_kmers = 0;
        r.sum_readK = r.sum_asmK = 0; r.ext_kstar = 0.0;
        mine.push_back(r);
      }
      mine.back().end = re[i];
      mine.back().n_kmers += re[i] - rs[i];
    }
    for (const mfx_region &r : mine) if (r.n_kmers >= min_kmers) raw.push_back(r);
    cls_reg[cls + 1] = raw.size();
  }
  mfx_rg_order(raw.data(), cls_reg, out);
}

// ---- device part: the class of a position, a wave's shares of its regions ----------------------------------------------------
#if defined(MFX_REGIONS_DEVICE)                               // the kernel files define it in front of this header
#include "mfx_track.h"                                        // mfx_trk_key: the monotone key of a double

// one valid k-mer's class (include/merfin_amd.h: the table at mfx_region), from the evaluation of -dump (merfin-dump.C:44-67)
__device__ __forceinline__ uint32_t mfx_rg_classify(double peak, uint32_t n_prob, const uint32_t *probK, const double *probP, double t,
                                                    uint32_t rv, uint32_t av, double &readK, double &x) {
  double prob;
  mfx_getK_core(peak, n_prob, probK, probP, rv, readK, prob);
  x = 0.0;
  if (readK == 0) return MFX_REGION_MISSING;
  if (av == 0) return MFX_RG_NONE;                            // readK / 0: not finite, in no class
  x = mfx_kmetric(readK, (double)av);
  if (x >= t) return MFX_REGION_COLLAPSED;
  if (x <= -t) return MFX_REGION_EXPANDED;
  return MFX_RG_NONE;
}

// the three words of the wave's 64 positions, stored by one lane: plain vector stores
__device__ __forceinline__ void mfx_rg_store_masks(uint64_t *planes, uint64_t nwords, uint64_t word, uint32_t cls) {
  const uint64_t m0 = __ballot(cls == MFX_REGION_MISSING), m1 = __ballot(cls == MFX_REGION_COLLAPSED), m2 = __ballot(cls == MFX_REGION_EXPANDED);
  if ((threadIdx.x & 63u) == 0u) {
    planes[word] = m0;
    planes[nwords + word] = m1;
    planes[2 * nwords + word] = m2;
  }
}

// The region of class `cls` that holds position p of `contig`: the last record of the class's sorted list that starts at or before it.
// ~0: none (its region fell to -minrun).  regs: 7 words a record -- contig | cls << 32, start, end, ...
__device__ __forceinline__ uint64_t mfx_rg_find(const uint64_t *regs, uint64_t lo, uint64_t hi, uint32_t contig, uint64_t p) {
  const uint64_t first = lo;
  while (lo < hi) {                                           // first record beyond (contig, p)
    const uint64_t mid = lo + (hi - lo) / 2;
    const uint32_t rc = (uint32_t)regs[mid * MFX_RG_REC_WORDS];
    const uint64_t rs = regs[mid * MFX_RG_REC_WORDS + 1];
    if (rc < contig || (rc == contig && rs <= p)) lo = mid + 1;
    else hi = mid;
  }
  if (lo == first) return ~0ull;
  const uint64_t r = lo - 1;
  if ((uint32_t)regs[r * MFX_RG_REC_WORDS] != contig || p >= regs[r * MFX_RG_REC_WORDS + 2]) return ~0ull;
  return r;
}

// A wave's flagged positions go to their regions.  Lanes of one region that are neighbours are added up first (the segmented shuffle
// reduce of mfx_track.h, over run numbers: equal neighbours only, so lanes of one region that another class separates send twice --
// every field is an integer sum or a maximum, the record is the same).  reg == ~0: the lane holds nothing.
__device__ __forceinline__ void mfx_rg_wave_add(uint64_t *regs, uint64_t *recount, uint64_t reg, uint64_t n, uint64_t sr, uint64_t sa, uint64_t key) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t prev = __shfl_up(reg, 1, 64);
  const bool head = lane == 0u || prev != reg;
  const uint64_t heads = __ballot(head);
  const uint32_t seg = (uint32_t)__popcll(heads & (~0ull >> (63u - lane)));      // the number of the lane's run of equal regions: does not decrease
#pragma unroll
  for (uint32_t off = 1; off < 64u; off <<= 1) {
    const uint32_t os = (uint32_t)__shfl_down((int)seg, off, 64);
    const uint64_t bn = __shfl_down(n, off, 64), bsr = __shfl_down(sr, off, 64), bsa = __shfl_down(sa, off, 64), bk = __shfl_down(key, off, 64);
    if (lane + off < 64u && os == seg) { n += bn; sr += bsr; sa += bsa; key = key > bk ? key : bk; }
  }
  if (head && reg != ~0ull) {
    unsigned long long *r = reinterpret_cast<unsigned long long *>(regs + reg * MFX_RG_REC_WORDS);
    (void)__hip_atomic_fetch_add(reinterpret_cast<unsigned long long *>(recount + reg), (unsigned long long)n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (sr) (void)__hip_atomic_fetch_add(r + 4, (unsigned long long)sr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (sa) (void)__hip_atomic_fetch_add(r + 5, (unsigned long long)sa, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (key) (void)__hip_atomic_fetch_max(r + 6, (unsigned long long)key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// One evaluated position of pass 2 (wave-wide call): its class again, its region, its share.  ok: a valid k-mer that pass 1 flagged.
__device__ __forceinline__ void mfx_rg_visit(const mfx_regions_args &a, uint32_t contig, uint64_t p, bool ok, uint32_t rv, uint32_t av) {
  uint64_t reg = ~0ull, n = 0, sr = 0, sa = 0, key = 0;
  if (ok) {
    double readK, x;
    const uint32_t cls = mfx_rg_classify(a.peak, a.n_prob, a.probK, a.probP, a.kstar, rv, av, readK, x);
    if (cls != MFX_RG_NONE) {
      const uint64_t lo = cls == MFX_REGION_MISSING ? a.reg_begin0 : cls == MFX_REGION_COLLAPSED ? a.reg_begin1 : a.reg_begin2;
      const uint64_t hi = cls == MFX_REGION_MISSING ? a.reg_begin1 : cls == MFX_REGION_COLLAPSED ? a.reg_begin2 : a.reg_begin3;
      reg = mfx_rg_find(a.regs, lo, hi, contig, p);
      if (reg != ~0ull) {
        n = 1;
        sa = av;
        if (cls != MFX_REGION_MISSING) {
          sr = (uint64_t)readK;                               // (integer-valued: 1, round(), probK[])
          key = cls == MFX_REGION_COLLAPSED ? mfx_trk_key(x) : ~mfx_trk_key(x);
        }
      }
    }
  }
  if (__any(reg != ~0ull)) mfx_rg_wave_add(a.regs, a.recount, reg, n, sr, sa, key);
}
#endif
